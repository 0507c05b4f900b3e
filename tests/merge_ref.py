"""Checker for the map-point merge on a map mirror, written from the reference -- MapManager::mergeMapPoints
(src/map_manager.cpp:801-882) with Frame::updateKeypointId (src/frame.cpp:380-402) -- over dicts and sets keyed by ids, one
function per pair (merge_pair), on the tables of a map as DeviceMap.download gives them.  Descriptors, covisibility, anchors
and nblms_ are not mirror state and are not modelled.  Two rules are the mirror stage's own: a pair with prev == new is
skipped (the reference would erase the point; neither of its callers passes such a pair), and whether the current frame
held prev (setMapPointObs(newlmid), :860-866) is an argument of the pair.

A map M is a dict:
  tables   the downloaded arrays, obs_lm and lm_state as the pairs so far left them (copies; everything else is shared)
  kfs      {kfid: set of lmids}     the live rows per keyframe: Frame::mapkps_ of the keyframes the map holds
  lms      {lmid: set of kfids}     the live rows per live landmark: MapPoint::set_kfids_
  row      {(kfid, lmid): row}      where the live observation stands in the table
  relabels {row: times relabelled}
"""
import numpy as np

LM_ALIVE, LM_3D, LM_OBS, LM_KP3D = 1, 2, 4, 8
OBS_ALIVE, OBS_STEREO = 1, 2
DONE, SKIP_RANGE, SKIP_SAME, SKIP_PREV_DEAD, SKIP_NEW_DEAD, SKIP_NEW_NOT3D = range(6)   # OV2_MERGE_* (include/ov2slam_hip.h)


def tables_of(m, spare=(8, 8)):
    """the tables a mirror of a synth_filter.make_map dict holds (as DeviceMap.from_filter_map fills them, rows in the dict's
    order), without a device: the `download` of a map that was never uploaded"""
    K, L, N = m["n_kf"] + spare[0], m["n_lm"] + spare[1], len(m["obs_kf"])
    seen = np.unique(m["obs_lm"])
    st = np.zeros(L, np.uint8)
    st[seen] = (LM_ALIVE | np.where(m["lm_3d"][seen] != 0, LM_3D, 0) | np.where(m["lm_isobs"][seen] != 0, LM_OBS, 0)
                | np.where(m["lm_kp3d"][seen] != 0, LM_KP3D, 0)).astype(np.uint8)
    xyz = np.zeros((L, 3))
    xyz[seen] = np.where((m["lm_3d"][seen] != 0)[:, None], m["lm_xyz"][seen], 0.0)
    pose = np.zeros((K, 7))
    pose[:m["n_kf"]] = m["poses"]
    kst = np.zeros(K, np.uint8)
    kst[:m["n_kf"]] = 1
    return dict(kf_pose=pose, kf_state=kst, lm_xyz=xyz, lm_state=st, obs_kf=m["obs_kf"].astype(np.int32), obs_lm=m["obs_lm"].astype(np.int32),
                obs_flag=np.full(N, OBS_ALIVE, np.uint8), obs_uv=m["obs_uv"].astype(np.float64), obs_ruv=np.zeros((N, 2)))


def build(d):
    """the map of downloaded tables; an observation counts when its row, its keyframe and its landmark are alive"""
    t = dict(d)
    t["obs_lm"], t["lm_state"] = d["obs_lm"].copy(), d["lm_state"].copy()
    kfs = {int(k): set() for k in np.flatnonzero(d["kf_state"])}
    lms = {int(l): set() for l in np.flatnonzero(d["lm_state"] & LM_ALIVE)}
    row = {}
    for i in np.flatnonzero(d["obs_flag"] & OBS_ALIVE).tolist():
        k, l = int(d["obs_kf"][i]), int(d["obs_lm"][i])
        if k in kfs and l in lms:
            assert (k, l) not in row, "a keyframe holds a landmark once"
            kfs[k].add(l); lms[l].add(k); row[(k, l)] = i
    return dict(tables=t, kfs=kfs, lms=lms, row=row, relabels={})


def merge_pair(M, p, n, cur_obs=False):
    """one MapManager::mergeMapPoints(p, n): returns (status, rows moved, rows in conflict)"""
    t, kfs, lms, row = M["tables"], M["kfs"], M["lms"], M["row"]
    L = len(t["lm_state"])
    if not (0 <= p < L and 0 <= n < L):
        return SKIP_RANGE, 0, 0
    if p == n:
        return SKIP_SAME, 0, 0
    if p not in lms:
        return SKIP_PREV_DEAD, 0, 0
    if n not in lms:
        return SKIP_NEW_DEAD, 0, 0
    if not t["lm_state"][n] & LM_3D:
        return SKIP_NEW_NOT3D, 0, 0
    moved = conflict = 0
    for k in sorted(lms[p]):
        i = row.pop((k, p))
        kfs[k].discard(p)
        if n in kfs[k]:          # Frame::updateKeypointId returns false: the keypoint keeps the id of a point that is gone
            conflict += 1
            continue
        t["obs_lm"][i] = n
        row[(k, n)] = i
        kfs[k].add(n); lms[n].add(k)
        M["relabels"][i] = M["relabels"].get(i, 0) + 1
        moved += 1
    del lms[p]
    t["lm_state"][p] = 0
    if cur_obs:
        t["lm_state"][n] |= LM_OBS
    return DONE, moved, conflict


def merge_list(M, pairs, cur_obs=None):
    """the pairs one after the other; returns (header dict, status bytes, per pair (status, moved, conflict))"""
    rec = [merge_pair(M, int(p), int(n), bool(cur_obs[i]) if cur_obs is not None else False) for i, (p, n) in enumerate(pairs)]
    done = sum(r[0] == DONE for r in rec)
    hdr = dict(n_pairs=len(rec), n_merged=done, n_skipped=len(rec) - done, n_rows_moved=sum(r[1] for r in rec),
               n_rows_conflict=sum(r[2] for r in rec))
    return hdr, np.array([r[0] for r in rec], np.uint8), rec


def canonical(M):
    """what device_map.canonical_state gives for the tables as they stand"""
    t = M["tables"]
    kfs = {k: tuple(t["kf_pose"][k]) for k in M["kfs"]}
    lms = {l: (tuple(t["lm_xyz"][l]), int(t["lm_state"][l])) for l in M["lms"]}
    obs = {o: int(t["obs_flag"][i] & OBS_STEREO) for o, i in M["row"].items()}
    return kfs, lms, obs


def row_dict(M):
    """(kfid, lmid) -> (uv, ruv, stereo flag) over the live rows"""
    t = M["tables"]
    return {o: (tuple(t["obs_uv"][i]), tuple(t["obs_ruv"][i]), int(t["obs_flag"][i] & OBS_STEREO)) for o, i in M["row"].items()}


def row_dict_of_tables(d):
    """the same from downloaded tables"""
    return row_dict(build(d))
