"""Seeded maps for the stereo-triangulation tests (Mapper::triangulateStereo, reference src/mapper.cpp:346-461): n_kf keyframes
of a stereo rig on a trajectory, the new keyframe last, so that every branch of the stage is reached.  numpy only.

The new keyframe holds landmarks that are already 3D, 2D landmarks without a stereo match, 2D stereo landmarks with a consistent
right pixel (0.3 px noise, depths 1-10 m, baseline 0.11 m) and mismatches: the right pixel moved by 6-40 px in a random direction,
a third of them to the wrong side of the left pixel.  With the rectified rig a wrong side is the negative-disparity exit and a
vertical offset the reprojection gate; its depth gate (fx b / |d| < 0.1 m) needs a disparity beyond 500 px, so a handful of
mismatches there are far ones: a left pixel near the right border matched to the left border.  With the general rig (a small
rotation between the cameras, other right intrinsics: the mid-point method) a wrong side gives diverging rays, the depth gate.
Older keyframes carry stereo rows too, also on landmarks that are still 2D: the stage must leave them alone.  Some rows and
some landmarks are dead."""
import numpy as np

from . import synth_ba, synth_scene

K4 = synth_scene.K4.copy()
W, H = 752, 480
BASELINE = 0.11


def rig_of(rectified, rng):
    """(Kr, Tlr): the right intrinsics and the right camera in the left frame (t then qx qy qz qw)"""
    if rectified:
        return K4.copy(), np.array([BASELINE, 0, 0, 0, 0, 0, 1.0])
    R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 0.008, 3)]))
    return K4 * np.array([1.01, 1.012, 1.0, 1.0]) + np.array([0, 0, 3.5, -2.25]), synth_ba.pose7(R, np.array([BASELINE, 0.003, -0.002]))


def _project(K, T, X):
    """pixels and depths of world points X in the camera at pose T (camera in the world)"""
    R = synth_ba.quat_to_rot(T[3:])
    pc = (X - T[:3]) @ R
    return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], -1), pc[:, 2]


def _compose(Twc, Tlr):
    """the right camera in the world: Twc * Tlr"""
    R, Rl = synth_ba.quat_to_rot(Twc[3:]), synth_ba.quat_to_rot(Tlr[3:])
    return synth_ba.pose7(R @ Rl, R @ Tlr[:3] + Twc[:3])


def make_map(n_kf=4, n_lm=1500, seed=0, rectified=True, noise_px=0.3, max_rows=None, new_frac=0.85):
    """returns a dict:
      n_kf, n_lm, K4 (left), Kr, Tlr, rectified, w, h, poses (n_kf, 7: t, qx qy qz qw), newkf = n_kf - 1
      rows sorted by (kf, lm): obs_kf, obs_lm (int32), obs_uv (n, 2 float32: Keypoint::unpx_), obs_stereo (uint8),
        obs_rpx (n, 2 float32: the right pixel, raw = undistorted for this rig; 0 without a match), obs_alive (uint8)
      lm_3d = lm_kp3d (n_lm uint8): MapPoint::is3d_ and Keypoint::is3d_ of its keypoints, lm_alive (uint8), lm_xyz (n_lm, 3): the
        true point, lm_kind (n_lm, str): '3d' | 'mono' | 'clean' | 'mismatch' | 'far' -- what its keypoint of the NEW keyframe is
      obs_rpx_true (n, 2 float64): the right pixel before noise, mismatch and rounding
    max_rows: rows of the older keyframes are dropped from the end until the table holds exactly this many
    new_frac: the share of the landmarks that the new keyframe sees (with more than one keyframe)"""
    rng = np.random.default_rng(seed)
    newkf = n_kf - 1
    Kr, Tlr = rig_of(rectified, rng)
    poses = np.zeros((n_kf, 7))
    for k in range(n_kf):
        R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 0.02, 3)]))
        poses[k] = synth_ba.pose7(R, np.array([0.12 * k, 0.0, 0.0]) + rng.normal(0, 0.015, 3))
    # points in front of the new keyframe, depths 1-10 m there, inside its left image
    z = rng.uniform(1.0, 10.0, n_lm)
    u, v = rng.uniform(12, W - 12, n_lm), rng.uniform(12, H - 12, n_lm)
    pc = np.stack([z * (u - K4[2]) / K4[0], z * (v - K4[3]) / K4[1], z], 1)
    X = pc @ synth_ba.quat_to_rot(poses[newkf, 3:]).T + poses[newkf, :3]

    kind = np.full(n_lm, "clean", dtype=object)
    q = rng.random(n_lm)
    kind[q < 0.30] = "3d"
    kind[(q >= 0.30) & (q < 0.40)] = "mono"
    kind[(q >= 0.75)] = "mismatch"
    if rectified:   # the depth gate of the disparity form: left pixel far right, right pixel at the left border
        far = np.flatnonzero((kind == "mismatch") & (u > K4[0] * BASELINE / 0.1 + 12))[:max(4, n_lm // 100)]
        kind[far] = "far"
    lm_3d = (kind == "3d").astype(np.uint8)
    in_new = rng.random(n_lm) < new_frac         # the others are seen by older keyframes only
    if n_kf == 1:
        in_new[:] = True
    lm_3d[~in_new] = rng.random(int((~in_new).sum())) < 0.5

    kf_l, lm_l, uv_l, st_l, rp_l, rt_l = [], [], [], [], [], []
    for k in range(n_kf):
        uv, zl = _project(K4, poses[k], X)
        ruv, zr = _project(Kr, _compose(poses[k], Tlr), X)
        ok = (zl > 0.5) & (zr > 0.5) & (uv[:, 0] > 8) & (uv[:, 0] < W - 8) & (uv[:, 1] > 8) & (uv[:, 1] < H - 8)
        ok &= (ruv[:, 0] > 8) & (ruv[:, 0] < W - 8) & (ruv[:, 1] > 8) & (ruv[:, 1] < H - 8)   # seen by both cameras
        ok &= in_new if k == newkf else (rng.random(n_lm) < 0.45)
        ids = np.flatnonzero(ok)
        n = len(ids)
        luv = uv[ids] + rng.normal(0, noise_px, (n, 2))
        rpx = ruv[ids] + rng.normal(0, noise_px, (n, 2))
        if k == newkf:
            kd = kind[ids]
            stereo = kd != "mono"
            stereo &= ~((kd == "3d") & (rng.random(n) < 0.3))           # some 3D keypoints have no match either
            mm = kd == "mismatch"
            ang = rng.uniform(0, 2 * np.pi, int(mm.sum()))
            rpx[mm] += np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(6, 40, (int(mm.sum()), 1))
            wrong = mm & (rng.random(n) < 0.33)                         # beyond the left pixel: the wrong side
            rpx[wrong, 0] = luv[wrong, 0] + rng.uniform(6, 40, int(wrong.sum()))
            fr = kd == "far"
            rpx[fr, 0] = rng.uniform(2, 8, int(fr.sum()))
        else:
            stereo = rng.random(n) < 0.5
        rpx = np.clip(rpx, 1.0, [W - 2.0, H - 2.0])
        rpx[~stereo] = 0.0
        kf_l.append(np.full(n, k, np.int32)); lm_l.append(ids.astype(np.int32)); uv_l.append(luv)
        st_l.append(stereo.astype(np.uint8)); rp_l.append(rpx); rt_l.append(ruv[ids])
    if max_rows is not None:
        n_new = len(kf_l[newkf])
        old = sum(len(a) for a in kf_l[:newkf])
        assert n_new < max_rows <= n_new + old, (n_new, old, max_rows)
        drop = n_new + old - max_rows
        for k in range(newkf - 1, -1, -1):
            d = min(drop, len(kf_l[k]))
            if d:
                kf_l[k], lm_l[k], uv_l[k], st_l[k], rp_l[k], rt_l[k] = (a[:len(a) - d] for a in (kf_l[k], lm_l[k], uv_l[k], st_l[k], rp_l[k], rt_l[k]))
            drop -= d
    obs_kf, obs_lm = np.concatenate(kf_l), np.concatenate(lm_l)
    obs_uv, obs_rpx = np.concatenate(uv_l).astype(np.float32), np.concatenate(rp_l).astype(np.float32)
    obs_stereo, obs_rpx_true = np.concatenate(st_l), np.concatenate(rt_l)
    obs_alive = (rng.random(len(obs_kf)) >= 0.03).astype(np.uint8)
    lm_alive = (rng.random(n_lm) >= 0.03).astype(np.uint8)
    return dict(n_kf=n_kf, n_lm=n_lm, K4=K4.copy(), Kr=Kr, Tlr=Tlr, rectified=bool(rectified), w=W, h=H, poses=poses, newkf=newkf,
                obs_kf=obs_kf, obs_lm=obs_lm, obs_uv=obs_uv, obs_stereo=obs_stereo, obs_rpx=obs_rpx, obs_alive=obs_alive,
                obs_rpx_true=obs_rpx_true, lm_3d=lm_3d, lm_kp3d=lm_3d.copy(), lm_alive=lm_alive, lm_xyz=X, lm_kind=kind)


def as_dicts(m):
    """the map as the plain dicts tests/stereo_tri_ref.py walks -- what lives of it: poses {kfid: pose7}, keypoints
    {kfid: {lmid: dict(unpx float32 (2,), is3d, stereo, runpx float32 (2,))}} (Frame::mapkps_), landmarks
    {lmid: dict(is3d, observers: sorted kfids)} (MapManager::map_plms_ with MapPoint::set_kfids_)"""
    poses = {k: m["poses"][k].copy() for k in range(m["n_kf"])}
    kps = {k: {} for k in poses}
    lms = {}
    for i, (k, l) in enumerate(zip(m["obs_kf"], m["obs_lm"])):
        k, l = int(k), int(l)
        if not m["obs_alive"][i] or not m["lm_alive"][l]:
            continue
        lms.setdefault(l, dict(is3d=bool(m["lm_3d"][l]), observers=[]))["observers"].append(k)
        kps[k][l] = dict(unpx=m["obs_uv"][i].copy(), is3d=bool(m["lm_kp3d"][l]), stereo=bool(m["obs_stereo"][i]),
                         runpx=m["obs_rpx"][i].copy())
    for l in lms:
        lms[l]["observers"].sort()
    return poses, kps, lms
