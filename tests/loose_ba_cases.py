"""Scenes for the looseBA tests: synth_ba.make_window maps edited so that the propagation has landmarks to move.

In a make_window map almost no landmark has a keyframe younger than the loop keyframe as its OLDEST observer, so the
landmark half of the propagation (src/optimizer.cpp:1571-1592) would never run.  A scene therefore takes `n_prop` landmarks
that at least two younger keyframes see and removes every observation of theirs by a keyframe <= nkfid -- on the host map,
on the device map and in the numpy snapshot alike, through the same hooks a live sequence uses.  A third of the landmarks
lose isobs_ (the culling can then remove them)."""
import numpy as np

from ov2slam_amd import device_map as DM
from ov2slam_amd import host_map, synth_ba

import loose_ba_ref as LR


def f32(P):
    """pixels rounded to float32, as Keypoint::unpx_ / runpx_ hold them (cv::Point2f)"""
    Q = P.copy()
    Q.res_uv = Q.res_uv.astype(np.float32).astype(np.float64)
    if Q.lm_anchor_uv is not None:
        Q.lm_anchor_uv = Q.lm_anchor_uv.astype(np.float32).astype(np.float64)
    return Q


def make_scene(n_kf=12, n_lm=600, ini=3, n=8, inv_depth=True, seed=35, n_prop=40, outlier_frac=0.08, obs_pick="nearest", min_younger=2, rm_kfs=()):
    """rm_kfs: keyframes removed from the map after the edits (MapManager::removeKeyframe / ov2_map_remove_keyframe)"""
    P = f32(synth_ba.make_window(n_kf, n_lm, inv_depth=inv_depth, seed=seed, max_obs=6, outlier_frac=outlier_frac, obs_pick=obs_pick))
    kf, lm, _, _, _ = DM.observations_of(P)
    younger = np.bincount(lm[kf > n], minlength=len(P.lm))
    older = np.bincount(lm[kf <= n], minlength=len(P.lm))
    pick = np.flatnonzero((younger >= min_younger) & (older >= 1))[:n_prop]
    sel = np.isin(lm, pick) & (kf <= n)
    return dict(P=P, ini=ini, n=n, inv_depth=inv_depth, rm_kf=kf[sel].copy(), rm_lm=lm[sel].copy(), prop_lm=pick,
                isobs_off=np.arange(0, len(P.lm), 3, dtype=np.int32), cur_kfid=n, rm_kfs=tuple(rm_kfs))


def build_host(s, stereo=True):
    hm = host_map.HostMap(s["P"], stereo=stereo)
    for k, l in zip(s["rm_kf"], s["rm_lm"]):
        hm.remove_obs(int(k), int(l))
    for l in s["isobs_off"]:
        hm.set_isobs(int(l), 0)
    hm.set_cur_frame(s["cur_kfid"])
    for k in s["rm_kfs"]:
        hm.remove_keyframe(k)
    return hm


def build_device(ctx, s, spare=(8, 8, 64)):
    dm = DM.DeviceMap.from_problem(ctx, s["P"], isobs="all", spare=spare)
    if len(s["rm_kf"]):
        dm.remove_obs(s["rm_kf"], s["rm_lm"])
    off = np.asarray(s["isobs_off"], np.int32)
    if len(off):
        dm.set_landmarks(off, None, np.full(len(off), DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D, np.uint8))
    for k in s["rm_kfs"]:
        dm.remove_keyframe(k)
    return dm


def snapshot(s):
    """the tables DeviceMap.download() gives for build_device(s), without a device"""
    P = s["P"]
    kf, lm, un, st, run = DM.observations_of(P)
    nk, nl = len(P.pose), len(P.lm)
    flag = (DM.OBS_ALIVE | (DM.OBS_STEREO * st.astype(np.uint8))).astype(np.uint8)
    gone = set(zip(s["rm_kf"].tolist(), s["rm_lm"].tolist()))
    for i, (k, l) in enumerate(zip(kf.tolist(), lm.tolist())):
        if (k, l) in gone:
            flag[i] = 0
    state = np.full(nl, DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D | DM.LM_OBS, np.uint8)
    state[np.asarray(s["isobs_off"], np.int64)] &= ~np.uint8(DM.LM_OBS)
    kf_state = np.ones(nk, np.uint8)
    kf_state[list(s["rm_kfs"])] = 0
    return dict(kf_pose=np.array(P.pose, np.float64).copy(), kf_state=kf_state, lm_xyz=DM.world_points_of(P), lm_state=state,
                obs_kf=kf.copy(), obs_lm=lm.copy(), obs_flag=flag, obs_uv=np.array(un, np.float64), obs_ruv=np.array(run, np.float64))


def block_keys(pb):
    return [(int(t), int(k), int(l)) for t, k, l in zip(pb["res_type"], pb["res_kfid"], pb["res_lmid"])]


def crafted(s, pb, seed=1):
    """a "solved" state and flags for the problem `pb` (any row order): the free poses moved by a few centimetres / tenths
    of a degree, the landmarks by a per cent, two inverse depths negative; flagged: one block in seven, every block of the
    loop keyframe's (= cur_kfid's) first rows among them, and the left blocks of ten landmarks without isobs_ (they end with
    one observer: isBad()).  Everything is keyed by ids, so two orders of one problem get the
    same state.  returns dict(pose: {kfid: 7}, lm: {lmid: values}, flags: set of (type, kfid, lmid))"""
    rng = np.random.default_rng(seed)
    pose = {}
    for k, c, p in sorted(zip(pb["pose_kfid"].tolist(), pb["pose_const"].tolist(), pb["pose"].tolist())):
        if c:
            pose[k] = np.array(p)
            continue
        dR, dt = synth_ba.se3_exp(np.concatenate([rng.normal(0, 0.03, 3), rng.normal(0, 0.004, 3)]))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = dR, dt
        pose[k] = LR.pose7(M @ LR.mat(np.array(p)))
    lm = {}
    for j, (l, v) in enumerate(sorted(zip(pb["lm_lmid"].tolist(), pb["lm"].tolist()))):
        v = np.array(v)
        lm[l] = v * (1 + rng.normal(0, 0.01)) if s["inv_depth"] else v + rng.normal(0, 0.02, 3)
        if s["inv_depth"] and j in (5, 17):
            lm[l] = -np.abs(lm[l])
    keys = sorted(set(block_keys(pb)))
    flags = {keys[i] for i in range(0, len(keys), 7)}
    flags |= set([k for k in keys if k[1] == s["cur_kfid"]][:12])
    # landmarks without isobs_ whose observers all lie in the problem: every left block but (XYZ) the first one flagged leaves
    # them one observer, the fewest observers first
    per_lm = {}
    for t, k, l in keys:
        if t in (LR.L_XYZ, LR.L_INV):
            per_lm.setdefault(l, []).append((t, k, l))
    nobs, _, _ = LR.observers(snapshot(s))
    extra = 1 if s["inv_depth"] else 0   # the anchor observation has no left block
    off = set(int(x) for x in s["isobs_off"])
    lonely = sorted((len(v), l) for l, v in per_lm.items() if l in off and len(v) + extra == nobs[l])
    for _, l in lonely[:10]:
        flags |= set(per_lm[l][0 if s["inv_depth"] else 1:])
    return dict(pose=pose, lm=lm, flags=flags)


def in_order(pb, cs):
    """the crafted state `cs` as arrays in the order of problem `pb`: (pose n x 7, lm n x e, flags n_res bytes)"""
    pose = np.array([cs["pose"][int(k)] for k in pb["pose_kfid"]]).reshape(-1, 7)
    lm = np.array([cs["lm"][int(l)] for l in pb["lm_lmid"]]).reshape(len(pb["lm_lmid"]), -1)
    flags = np.array([k in cs["flags"] for k in block_keys(pb)], np.uint8)
    return pose, lm, flags
