"""numpy checker of the local-map selection (ov2_map_local_ids_batch, csrc/map.hip; MapManager::updateFrameCovisibility,
src/map_manager.cpp:117-193, and the set assembly of Mapper::matchingToLocalMap, src/mapper.cpp:475-517): plain set algebra on
a table dump in the layout of DeviceMap.download() -- kf_state, lm_state, obs_kf, obs_lm, obs_flag -- and a dict of the stored
sets {kfid: ids}.  Only integers come out.  tests/test_local_ids_ref_cpu.py checks it against the C++ host stage."""
import numpy as np

LM_ALIVE, LM_3D, LM_OBS, LM_KP3D = 1, 2, 4, 8
OBS_ALIVE = 1


def live_rows(d):
    """(kf, lm) of the live rows: the row, its keyframe and its landmark are alive"""
    kf, lm = np.asarray(d["obs_kf"], np.int64), np.asarray(d["obs_lm"], np.int64)
    live = (np.asarray(d["obs_flag"]) & OBS_ALIVE).astype(bool)
    if len(live):
        live &= np.asarray(d["kf_state"])[kf].astype(bool) & (np.asarray(d["lm_state"])[lm] & LM_ALIVE).astype(bool)
    return kf[live], lm[live]


def local_ids(d, sets, k, extend, nmax_local):
    """the record of keyframe k: dict(cov_kfid, cov_score, oldest_cov, n_fresh, swapped, extended, lmid, fresh).  `sets` is
    not changed; the caller stores lmid as the set of k where a sequence of calls is replayed"""
    kf, lm = live_rows(d)
    obs_k = set(lm[kf == k].tolist())
    cov = {}
    for j, l in zip(kf.tolist(), lm.tolist()):
        if j != k and l in obs_k:
            cov[j] = cov.get(j, 0) + 1
    C = sorted(cov)
    state = np.asarray(d["lm_state"])
    S = {l for j, l in zip(kf.tolist(), lm.tolist()) if j in cov and (state[l] & LM_KP3D) and l not in obs_k}
    old = set(int(l) for l in sets.get(k, ()))
    swapped = 2 * len(S) > len(old)
    cur = set(S) if swapped else old | S
    extended = bool(extend) and len(C) > 0 and len(cur) < nmax_local
    if extended:
        cur |= set(int(l) for l in sets.get(C[0], ()))
    return dict(cov_kfid=C, cov_score=[cov[j] for j in C], oldest_cov=C[0] if C else -1, n_fresh=len(S), swapped=int(swapped),
                extended=int(extended), lmid=sorted(cur), fresh=sorted(S))
