"""Checker of the temporal-triangulation stage: Mapper::triangulateTemporal (reference src/mapper.cpp:191-344) restated over
plain dicts, written from the reference -- not from the C++ host stage or the kernel.  The per-pair body (mid-point
triangulation, gates, world point, parallax) is the oracle's (oracle_py.triangulate_pairs); selection, relative poses,
bearings and the margins to every threshold are numpy here.

Inputs (ov2slam_amd.synth_temporal.as_dicts): poses {kfid: [t, qx qy qz qw]} of the keyframes that exist, keypoints
{kfid: {lmid: (unpx float32 (2,), is3d)}} (Frame::mapkps_), landmarks {lmid: dict(is3d, observers)} (MapManager::map_plms_
with MapPoint::set_kfids_).  Nothing is modified."""
import numpy as np

from ov2slam_amd import synth_ba

# the branch a keypoint takes, in the reference's order (the values of ov2::TemporalBranch)
NO_MAPPOINT, ALREADY_3D, FEW_OBSERVERS, OLDEST_IS_NEW, KF_GONE, NO_MOTION, KP_MISSING, GOOD, BEHIND_REMOVED, BEHIND_KEPT, \
    REPROJ_REMOVED, REPROJ_KEPT = range(12)
BRANCH_NAMES = ("no_mappoint", "already_3d", "few_observers", "oldest_is_new", "kf_gone", "no_motion", "kp_missing", "good",
                "behind_removed", "behind_kept", "reproj_removed", "reproj_kept")
REMOVES = (NO_MAPPOINT, BEHIND_REMOVED, REPROJ_REMOVED)

# the maps of the GPU tests (tests/test_temporal_gpu.py): keyframes, landmarks, seed -- each with stereo on and off.  The CPU
# test asserts that none of their keypoints stands within 1e-6 (relative) of a threshold.
GPU_CASES = [(nk, nl, seed) for nk, nl in ((4, 300), (8, 1500), (12, 4000)) for seed in (11, 12, 13)]
MAX_REPROJ_ERR = 3.0


def _Rt(T):
    return synth_ba.quat_to_rot(np.asarray(T[3:], np.float64)), np.asarray(T[:3], np.float64)


def bearing(unpx, K):
    """Frame::computeKeypoint (src/frame.cpp:246-254): iK * [unpx, 1] normalised, unpx a float pixel"""
    b = np.array([(float(unpx[0]) - K[2]) / K[0], (float(unpx[1]) - K[3]) / K[1], 1.0])
    return b / np.linalg.norm(b)


def _rel(x, thr):
    return abs(x - thr) / thr


def triangulate_temporal(O, poses, kps, lms, newkf, K, stereo, max_reproj_err):
    """returns a list, one dict per 2D keypoint of keyframe newkf in ascending lmid order:
      lmid, branch, and for candidates: kfid (the source keyframe), baseline, pt_a, wpt, invdepth, parallax, status
      margin: the smallest relative distance |x - thr| / thr to any threshold the keypoint met on its way
              (0.01 m, 0.1 m depth in either view, max_reproj_err in either view, 20 px); inf if it met none"""
    K = np.asarray(K, np.float64)
    Rj, tj = _Rt(poses[newkf])
    out, cand = [], []
    rel = {}                                      # source keyframe -> (R, t) of Tcicj, pose pair index
    for lmid in sorted(l for l, (_, is3d) in kps[newkf].items() if not is3d):      # Frame::getKeypoints2d
        r = dict(lmid=lmid, margin=np.inf)
        out.append(r)
        lm = lms.get(lmid)
        if lm is None:
            r["branch"] = NO_MAPPOINT; continue
        if lm["is3d"]:
            r["branch"] = ALREADY_3D; continue
        obs = sorted(lm["observers"])
        if len(obs) < 2:
            r["branch"] = FEW_OBSERVERS; continue
        kfid = obs[0]
        if kfid == newkf:
            r["branch"] = OLDEST_IS_NEW; continue
        if kfid not in poses:
            r["branch"] = KF_GONE; continue
        if kfid not in rel:
            Ri, ti = _Rt(poses[kfid])
            rel[kfid] = (Ri.T @ Rj, Ri.T @ (tj - ti), len(rel))                    # Tcicj = Tciw * Twcj
        R, t, g = rel[kfid]
        r["kfid"], r["baseline"] = kfid, float(np.linalg.norm(t))
        if stereo:
            r["margin"] = min(r["margin"], _rel(r["baseline"], 0.01))
            if r["baseline"] < 0.01:
                r["branch"] = NO_MOTION; continue
        if lmid not in kps[kfid]:
            r["branch"] = KP_MISSING; continue
        r["bva"], r["bvb"] = bearing(kps[kfid][lmid][0], K), bearing(kps[newkf][lmid][0], K)   # Keypoint::bv_
        r["ua"], r["ub"] = np.float32(kps[kfid][lmid][0]), np.float32(kps[newkf][lmid][0])      # Keypoint::unpx_
        r["g"] = g
        cand.append(r)
    if not cand:
        return out
    order = sorted(rel, key=lambda k: rel[k][2])
    T_ab = np.stack([synth_ba.pose7(rel[k][0], rel[k][1]) for k in order])
    Twc_a = np.stack([np.asarray(poses[k], np.float64) for k in order])
    ua, ub = np.stack([r["ua"] for r in cand]), np.stack([r["ub"] for r in cand])
    bva, bvb = np.stack([r["bva"] for r in cand]), np.stack([r["bvb"] for r in cand])
    res = O.triangulate_pairs(T_ab, bva, bvb, ua, ub, K, K, max_reproj_err, method=0, Twc_a=Twc_a,
                              grp=np.array([r["g"] for r in cand], np.int32), want_parallax=True)
    for i, r in enumerate(cand):
        R, t, _ = rel[r["kfid"]]
        X = res["pt_a"][i]
        Xb = R.T @ (X - t)                                                          # Tcjci * left_pt
        st, par = int(res["status"][i]), float(res["parallax"][i])
        r.update(pt_a=X, wpt=res["wpt"][i], invdepth=1.0 / X[2], parallax=par, status=st)
        m = min(r["margin"], _rel(X[2], 0.1), _rel(Xb[2], 0.1))
        assert (st == 1) == (X[2] < 0.1 or Xb[2] < 0.1)
        if st != 1:
            def dist(P, u):   # |projCamToImage(P) - unpx|: float pixels, float distance
                px = np.float32(K[:2] * (P[:2] * (1.0 / P[2])) + K[2:])
                d = px - u
                return float(np.float32(np.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]))))
            ld, rd = dist(X, r["ua"]), dist(Xb, r["ub"])
            r["ldist"], r["rdist"] = ld, rd
            m = min(m, _rel(ld, max_reproj_err), _rel(rd, max_reproj_err))
            assert (st == 2) == (ld > np.float32(max_reproj_err) or rd > np.float32(max_reproj_err)) or m < 1e-6
        if st == 0:
            r["branch"] = GOOD
        else:
            m = min(m, _rel(par, 20.0))
            r["branch"] = (BEHIND_REMOVED if par > 20.0 else BEHIND_KEPT) if st == 1 else (REPROJ_REMOVED if par > 20.0 else REPROJ_KEPT)
        r["margin"] = m
    return out


def parallax_independent(poses, kfid, newkf, ua, ub, K):
    """rotation-compensated parallax by another route: the new keyframe's pixel is mapped through the infinite homography
    K R K^-1 of the relative rotation, then compared with the older pixel"""
    K = np.asarray(K, np.float64)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    Ri, Rj = _Rt(poses[kfid])[0], _Rt(poses[newkf])[0]
    h = Km @ (Ri.T @ Rj) @ np.linalg.inv(Km) @ np.array([float(ub[0]), float(ub[1]), 1.0])
    return float(np.linalg.norm(h[:2] / h[2] - np.asarray(ua, np.float64)))
