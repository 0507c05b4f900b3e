"""Optimizer::looseBA (reference src/optimizer.cpp:900-1672) in plain numpy on a table snapshot of the map mirror
(DeviceMap.download() layout: kf_pose, kf_state, lm_xyz, lm_state, obs_kf, obs_lm, obs_flag, obs_uv, obs_ruv): the range
selection of its set-up (:985-1270) and the six steps of its update (:1330-1657).  Written from the reference's text; the
kernels of csrc/map.hip and the host stage Optimizer::setupRangeBA / applyLooseBA are what it checks.

Mirror conventions (include/ov2slam_hip.h): a row counts when its flag, its keyframe and its landmark are alive;
MapPoint::kfid_ is the landmark's oldest live observer; MapPoint::isBad() is
(observers < 2 and not isobs_ and is3d_) or (observers == 0 and not isobs_), and clears is3d_ when it answers true."""
import numpy as np

LM_ALIVE, LM_3D, LM_OBS, LM_KP3D = 1, 2, 4, 8
OBS_ALIVE, OBS_STEREO = 1, 2
L_XYZ, R_XYZ, L_INV, R_INV, RANCH_INV = range(5)


def copy_state(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def live_rows(d):
    live = (d["obs_flag"] & OBS_ALIVE).astype(bool)
    if len(live):
        live &= d["kf_state"][d["obs_kf"]].astype(bool) & (d["lm_state"][d["obs_lm"]] & LM_ALIVE).astype(bool)
    return live


def observers(d):
    """per landmark: the number of live observers, the oldest one (-1: none) and its row"""
    L = len(d["lm_state"])
    rows = np.flatnonzero(live_rows(d))
    nobs = np.bincount(d["obs_lm"][rows], minlength=L)
    oldest, orow = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    order = rows[np.lexsort((rows, d["obs_kf"][rows]))][::-1]   # descending (kf, row): the last write is the smallest kfid
    oldest[d["obs_lm"][order]] = d["obs_kf"][order]
    orow[d["obs_lm"][order]] = order
    return nobs, oldest, orow


def is_bad(state, nobs):
    isobs = (state & LM_OBS) != 0
    return ((nobs < 2) & ~isobs & ((state & LM_3D) != 0)) | ((nobs == 0) & ~isobs)


# ---- SE(3) on (t, q = x y z w) ------------------------------------------------------------------------------------
def rot(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def mat(p7):
    M = np.eye(4)
    M[:3, :3] = rot(p7[3:])
    M[:3, 3] = p7[:3]
    return M


def quat(R):
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        return np.array([0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s])
    if R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        return np.array([(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s])
    s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
    return np.array([(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s])


def pose7(M):
    return np.concatenate([M[:3, 3], quat(M[:3, :3])])


def inv(M):
    out = np.eye(4)
    out[:3, :3] = M[:3, :3].T
    out[:3, 3] = -M[:3, :3].T @ M[:3, 3]
    return out


# ---- set-up (:985-1270) -------------------------------------------------------------------------------------------
def setup(d, inikfid, nkfid, nmin_cst_kfs, inv_depth):
    """the flat problem of looseBA(inikfid, nkfid, .) keyed like device_map.fetch_view (ids, ascending kfid / lmid, residual
    blocks in row order), and the state after the set-up (isBad() landmarks have lost LM_3D).  returns (problem, state)"""
    d = copy_state(d)
    K = len(d["kf_state"])
    role = np.zeros(K, np.int64)   # 0 outside, 1 optimised, 2 constant
    ncst = 0
    for k in range(max(inikfid, 0), min(nkfid, K - 1) + 1):
        if not d["kf_state"][k]:
            continue
        if ncst < nmin_cst_kfs:
            role[k], ncst = 2, ncst + 1
        else:
            role[k] = 1
    live = live_rows(d)
    nobs, _, _ = observers(d)
    okf, olm = d["obs_kf"], d["obs_lm"]
    cand = np.unique(olm[live & (role[okf] == 1) & ((d["lm_state"][olm] & LM_KP3D) != 0)])
    bad = cand[is_bad(d["lm_state"][cand], nobs[cand])]
    d["lm_state"][bad] &= ~np.uint8(LM_3D)
    local = np.zeros(len(d["lm_state"]), bool)
    local[cand] = True
    local[bad] = False
    use = live & local[olm] & (okf <= nkfid)          # younger observers are left out (:1056)
    role[np.unique(okf[use])] = np.where(role[np.unique(okf[use])] == 0, 2, role[np.unique(okf[use])])
    anchor = np.full(len(local), -1, np.int64)
    for i in np.flatnonzero(use):
        if anchor[olm[i]] < 0 or okf[i] < anchor[olm[i]]:
            anchor[olm[i]] = okf[i]
    pose_kfid = np.flatnonzero(role).astype(np.int32)
    lm_lmid = np.flatnonzero(local & (anchor >= 0 if inv_depth else True)).astype(np.int32)
    lm = np.zeros((len(lm_lmid), 1 if inv_depth else 3))
    auv, akf = np.zeros((len(lm_lmid), 2)), np.full(len(lm_lmid), -1, np.int32)
    idx = {int(l): q for q, l in enumerate(lm_lmid)}
    if not inv_depth:
        lm[:] = d["lm_xyz"][lm_lmid]
    rt, rk, rl, ruv = [], [], [], []
    for i in np.flatnonzero(use):
        k, l = int(okf[i]), int(olm[i])
        if l not in idx:
            continue
        stereo = bool(d["obs_flag"][i] & OBS_STEREO)
        if inv_depth and anchor[l] == k:
            q = idx[l]
            pc = inv(mat(d["kf_pose"][k])) @ np.append(d["lm_xyz"][l], 1.0)
            lm[q, 0], akf[q], auv[q] = 1.0 / pc[2], k, d["obs_uv"][i]
            if stereo:
                rt.append(RANCH_INV); rk.append(k); rl.append(l); ruv.append(d["obs_ruv"][i])
            continue
        rt.append(L_INV if inv_depth else L_XYZ); rk.append(k); rl.append(l); ruv.append(d["obs_uv"][i])
        if stereo:
            rt.append(R_INV if inv_depth else R_XYZ); rk.append(k); rl.append(l); ruv.append(d["obs_ruv"][i])
    pb = dict(aborted=False, pose_kfid=pose_kfid, pose_const=(role[pose_kfid] == 2).astype(np.uint8), pose=d["kf_pose"][pose_kfid].copy(),
              lm_lmid=lm_lmid, lm=lm, lm_anchor_kfid=akf, lm_anchor_uv=auv, res_type=np.array(rt, np.uint8),
              res_kfid=np.array(rk, np.int32), res_lmid=np.array(rl, np.int32), res_uv=np.array(ruv, np.float64).reshape(-1, 2),
              bad_lmid=np.sort(bad).astype(np.int32))
    return pb, d


# ---- update (:1330-1657) ------------------------------------------------------------------------------------------
def update(d, pb, pose, lm, outlier, nkfid, cur_kfid, K4, inv_depth):
    """the six steps on the state `d` (as the set-up left it, or edited since), from the problem `pb` of setup(), its solved
    poses (n_pose x 7) and landmarks, and the per-block flags.  returns (state, counts, T_corr as a 4 x 4 matrix)"""
    d = copy_state(d)
    c = dict(ran=0, n_flagged_left=0, n_flagged_right=0, n_removed_obs=0, n_stereo_off=0, n_removed_lm=0, n_written=0, n_propagated=0,
             n_kf_younger=0, n_bad=0)
    if len(pb["res_type"]) == 0:
        return d, c, np.eye(4)
    c["ran"] = 1
    pose, lm, outlier = np.asarray(pose, np.float64).reshape(-1, 7), np.asarray(lm, np.float64), np.asarray(outlier).astype(bool)
    lm = lm.reshape(len(pb["lm_lmid"]), -1)
    pidx = {int(k): i for i, k in enumerate(pb["pose_kfid"])}
    # 1. constants
    old = d["kf_pose"].copy()
    ini, opt = inv(mat(old[nkfid])), mat(pose[pidx[nkfid]])
    T_corr = opt @ ini
    # 2. local landmarks, observers as they are before any removal
    nobs, oldest, orow = observers(d)
    badset = set(int(l) for l in pb["bad_lmid"])
    local = set(int(l) for l in pb["lm_lmid"])
    for q, l in enumerate(pb["lm_lmid"]):
        l = int(l)
        st = d["lm_state"][l]
        if not (st & LM_ALIVE):
            continue
        if is_bad(np.uint8(st), nobs[l]):
            d["lm_state"][l] = st & ~np.uint8(LM_3D)
            badset.add(l)
            continue
        if inv_depth:
            z = 1.0 / lm[q, 0]
            a = int(oldest[l])
            if z <= 0.0 or a not in pidx:
                badset.add(l)
                continue
            u, v = d["obs_uv"][orow[l]]
            w = mat(old[a]) @ np.array([z * (u - K4[2]) / K4[0], z * (v - K4[3]) / K4[1], z, 1.0])
            d["lm_xyz"][l] = w[:3]
        else:
            d["lm_xyz"][l] = lm[q]
        d["lm_state"][l] = st | LM_3D | LM_KP3D
        c["n_written"] += 1
    # 3. landmarks anchored by a keyframe younger than the loop keyframe
    for l in np.flatnonzero(((d["lm_state"] & LM_ALIVE) != 0) & ((d["lm_state"] & LM_KP3D) != 0) & (oldest > nkfid)):
        if int(l) in local:
            continue
        A = mat(old[oldest[l]])
        w = (opt @ (ini @ A)) @ (inv(A) @ np.append(d["lm_xyz"][l], 1.0))
        d["lm_xyz"][l] = w[:3]
        d["lm_state"][l] |= LM_3D
        c["n_propagated"] += 1
    # 4. poses
    for i, k in enumerate(pb["pose_kfid"]):
        if not pb["pose_const"][i] and d["kf_state"][k]:
            d["kf_pose"][k] = pose[i]
    for k in np.flatnonzero(d["kf_state"]):
        if k > nkfid:
            d["kf_pose"][k] = pose7(opt @ (ini @ mat(old[k])))
            c["n_kf_younger"] += 1
    # 5. flagged blocks, over the rows of the set-up
    row_of = {(int(k), int(l)): i for i, (k, l) in enumerate(zip(d["obs_kf"], d["obs_lm"])) if d["obs_flag"][i] & OBS_ALIVE}
    left, right = set(), set()
    for t, k, l, f in zip(pb["res_type"], pb["res_kfid"], pb["res_lmid"], outlier):
        if not f:
            continue
        if t in (L_XYZ, L_INV):
            left.add((int(k), int(l))); c["n_flagged_left"] += 1
        else:
            right.add((int(k), int(l))); c["n_flagged_right"] += 1
        badset.add(int(l))
    live = live_rows(d)
    for (k, l) in right - left:
        i = row_of.get((k, l))
        if i is not None and live[i] and d["obs_flag"][i] & OBS_STEREO:
            d["obs_flag"][i] &= ~np.uint8(OBS_STEREO)
            c["n_stereo_off"] += 1
    for (k, l) in left:
        i = row_of.get((k, l))
        if i is not None and live[i]:
            d["obs_flag"][i] = 0
            c["n_removed_obs"] += 1
        if k == cur_kfid:
            d["lm_state"][l] &= ~np.uint8(LM_OBS)
    # 6. culling over the bad set, observers counted again
    nobs, oldest, _ = observers(d)
    c["n_bad"] = len(badset)
    for l in sorted(badset):
        st = d["lm_state"][l]
        if not (st & LM_ALIVE):
            continue
        if is_bad(np.uint8(st), nobs[l]) or (nobs[l] < 3 and oldest[l] < nkfid - 3 and not (st & LM_OBS)):
            d["lm_state"][l] = 0
            c["n_removed_lm"] += 1
    return d, c, T_corr


def canonical(d):
    """device_map.canonical_state with poses as 4 x 4 matrices (q and -q are one rotation)"""
    kfs = {int(k): mat(d["kf_pose"][k]) for k in np.flatnonzero(d["kf_state"])}
    lms = {int(l): (d["lm_xyz"][l].copy(), int(d["lm_state"][l])) for l in np.flatnonzero(d["lm_state"] & LM_ALIVE)}
    live = live_rows(d)
    obs = {(int(k), int(l)): int(f & OBS_STEREO) for k, l, f in zip(d["obs_kf"][live], d["obs_lm"][live], d["obs_flag"][live])}
    return kfs, lms, obs
