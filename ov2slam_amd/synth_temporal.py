"""Seeded maps for the temporal-triangulation tests (Mapper::triangulateTemporal, reference src/mapper.cpp:191-344): K >= 4
keyframes on a trajectory, pinhole intrinsics, landmarks observed by runs of keyframes, so that every branch of the stage
is reached.  numpy only.

The new keyframe is the one BEFORE the last: a landmark it sees first and the last keyframe sees too has
two observers with the new keyframe as the oldest (:264-266).  The new keyframe stands 5 mm from an older one (`near_kf`:
the camera came back), so the landmarks that one saw first meet the stereo-only no-motion test (:287).  A map with dangling
references holds one keyframe more than the K asked for, kfid 0, which is then culled: the landmarks it saw first still
list it (:268-271), and the K keyframes that exist keep at least one older keyframe that gives candidates with either
setting of the stereo flag, at K = 4 too.
"""
import numpy as np

from . import synth_ba, synth_scene

K4 = synth_scene.K4.copy()
W, H = 752, 480


def _project(T, X):
    R = synth_ba.quat_to_rot(T[3:])
    pc = (X - T[:3]) @ R
    return np.stack([K4[0] * pc[:, 0] / pc[:, 2] + K4[2], K4[1] * pc[:, 1] / pc[:, 2] + K4[3]], -1), pc[:, 2]


def make_map(n_kf=8, n_lm=1000, seed=0, noise_px=0.3, dangling=True):
    """returns a dict:
      n_kf: the number of kfids, 0 .. n_kf - 1: the n_kf asked for, and with dangling=True one more, the culled kfid 0
      K4, w, h, poses (n_kf, 7: t, qx qy qz qw), newkf, near_kf (the keyframe < 1 cm from newkf)
      obs_kf, obs_lm (int32), obs_uv (n, 2 float32: Keypoint::unpx_), sorted by (kf, lm); obs_uv64: the same before rounding
      lm_3d, lm_kp3d (n_lm uint8): MapPoint::is3d_ / Keypoint::is3d_ of its keypoints; lm_xyz (n_lm, 3): the true point
      lm_kind (n_lm, str): 'clean' | '3d' | '3d_kp2d' | 'reproj' | 'behind'
      forget_lm, forget_kf, forget_kp ((kf, lm) pairs): applied after the map is built, they leave keypoints without a map
        point, observers without a keyframe and observers without a keypoint (dangling=False: none of the three, for maps
        that a device mirror has to represent: an observation is live there only with its keyframe and landmark)
    Depths stay <= 10 m and keyframes other than near_kf stand >= 5 cm from the new one."""
    assert n_kf >= 4
    n_all = n_kf + int(dangling)                 # kfid 0 is the culled keyframe of a dangling map
    rng = np.random.default_rng(seed)
    newkf = n_all - 2
    near_kf = max(newkf - 2, 1)
    poses = np.zeros((n_all, 7))
    for k in range(n_all):
        R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 0.02, 3)]))
        t = np.array([0.12 * k, 0.0, 0.0]) + rng.normal(0, 0.015, 3)
        poses[k] = synth_ba.pose7(R, t)
    # the camera is back where keyframe near_kf stood, 5 mm beside it
    d = rng.normal(0, 1, 3)
    poses[newkf, :3] = poses[near_kf, :3] + 0.005 * d / np.linalg.norm(d)
    for k in range(n_all):
        if k not in (newkf, near_kf):
            assert np.linalg.norm(poses[k, :3] - poses[newkf, :3]) >= 0.05

    X = np.stack([rng.uniform(-2.5, 2.5 + 0.12 * n_all, n_lm), rng.uniform(-1.6, 1.6, n_lm), rng.uniform(2.0, 9.5, n_lm)], 1)
    first = rng.integers(int(dangling), newkf + 1, n_lm)   # a landmark the new keyframe never saw is of no use here
    last = np.minimum(first + rng.integers(0, n_all, n_lm), n_all - 1)
    u = rng.random(n_lm)
    first[u < 0.06] = newkf                      # first seen by the new keyframe ...
    last[u < 0.03] = newkf                       # ... alone, or with the last keyframe
    last[(u >= 0.03) & (u < 0.06)] = n_all - 1
    sel = (u >= 0.06) & (u < 0.14)               # seen first by the keyframe the camera came back to
    first[sel] = near_kf
    last[sel] = np.maximum(last[sel], newkf)
    sel = (u >= 0.14) & (u < 0.55)               # runs that reach the new keyframe
    last[sel] = np.maximum(last[sel], newkf)
    if dangling:                                 # seen first by the keyframe that is culled afterwards
        sel = (u >= 0.55) & (u < 0.61)
        first[sel] = 0
        last[sel] = np.maximum(last[sel], newkf)
    kind = np.full(n_lm, "clean", dtype=object)
    v = rng.random(n_lm)
    kind[v < 0.35] = "3d"
    kind[(v >= 0.35) & (v < 0.37)] = "3d_kp2d"
    kind[(v >= 0.37) & (v < 0.47)] = "reproj"
    kind[(v >= 0.47) & (v < 0.57)] = "behind"

    obs_kf, obs_lm, obs_uv = [], [], []
    uv_true = np.zeros((n_all, n_lm, 2))
    vis = np.zeros((n_all, n_lm), bool)
    for k in range(n_all):
        uv, z = _project(poses[k], X)
        uv_true[k] = uv
        vis[k] = (first <= k) & (k <= last) & (z > 0.5) & (uv[:, 0] > 8) & (uv[:, 0] < W - 8) & (uv[:, 1] > 8) & (uv[:, 1] < H - 8)
    oldest = np.where(vis.any(0), vis.argmax(0), -1)
    for k in range(n_all):
        ids = np.flatnonzero(vis[k])
        uv = uv_true[k, ids] + rng.normal(0, noise_px, (len(ids), 2))
        if k == newkf:   # gross outliers in the new keyframe's pixel
            o = oldest[ids]
            flow = uv_true[k, ids] - uv_true[np.maximum(o, 0), ids]            # pixel motion since the oldest observer
            nf = np.linalg.norm(flow, axis=1, keepdims=True) + 1e-9
            perp = np.stack([-flow[:, 1], flow[:, 0]], 1) / nf
            rp = kind[ids] == "reproj"                                             # off the epipolar line: reprojection gate
            uv[rp] += perp[rp] * (rng.uniform(8, 30, (rp.sum(), 1)) * rng.choice([-1.0, 1.0], (rp.sum(), 1)))
            bh = kind[ids] == "behind"                                             # moved against the flow: the rays diverge
            uv[bh] = uv_true[np.maximum(o, 0), ids][bh] - flow[bh] / nf[bh] * rng.uniform(3, 60, (bh.sum(), 1))
            uv = np.clip(uv, 1.0, [W - 2.0, H - 2.0])
        obs_kf.append(np.full(len(ids), k, np.int32)); obs_lm.append(ids.astype(np.int32)); obs_uv.append(uv)
    obs_kf, obs_lm, obs_uv64 = np.concatenate(obs_kf), np.concatenate(obs_lm), np.concatenate(obs_uv)
    obs_uv = obs_uv64.astype(np.float32)

    lm_3d = np.isin(kind, ("3d", "3d_kp2d")).astype(np.uint8)
    lm_kp3d = (kind == "3d").astype(np.uint8)
    forget_lm, forget_kf, forget_kp = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32)
    if dangling:
        two_d = (lm_3d == 0) & vis[newkf] & (vis.sum(0) >= 2) & (oldest < newkf)
        pool = rng.permutation(np.flatnonzero(two_d))
        n = max(2, len(pool) // 25)
        forget_lm = np.sort(pool[:n]).astype(np.int32)
        kp = pool[n:2 * n]
        kp = kp[oldest[kp] != 0]
        forget_kp = np.stack([oldest[kp], kp], 1).astype(np.int32)
        forget_kf = np.array([0], np.int32)      # the first keyframe is gone (culled), its landmarks still list it
        assert near_kf != 0 and newkf != 0
    return dict(K4=K4.copy(), w=W, h=H, poses=poses, newkf=newkf, near_kf=near_kf, obs_kf=obs_kf, obs_lm=obs_lm, obs_uv=obs_uv,
                obs_uv64=obs_uv64,
                lm_3d=lm_3d, lm_kp3d=lm_kp3d, lm_xyz=X, lm_kind=kind, forget_lm=forget_lm, forget_kf=forget_kf, forget_kp=forget_kp,
                n_kf=n_all, n_lm=n_lm)


def as_dicts(m, exact_px=False):
    """the map as the plain dicts tests/temporal_ref.py walks -- after the forget_* edits: poses {kfid: pose7} of the keyframes
    that exist, keypoints {kfid: {lmid: (unpx float32 (2,), is3d)}}, landmarks {lmid: dict(is3d, observers: sorted kfids)}.
    exact_px: the pixels before their rounding to float (float64), for checks of the geometry alone"""
    gone_kf = set(int(k) for k in m["forget_kf"])
    poses = {k: m["poses"][k].copy() for k in range(m["n_kf"]) if k not in gone_kf}
    kps = {k: {} for k in poses}
    lms = {}
    for k, l, uv in zip(m["obs_kf"], m["obs_lm"], m["obs_uv64" if exact_px else "obs_uv"]):
        k, l = int(k), int(l)
        lms.setdefault(l, dict(is3d=bool(m["lm_3d"][l]), observers=[]))["observers"].append(k)
        if k in kps:
            kps[k][l] = (uv.copy(), bool(m["lm_kp3d"][l]))
    for l in lms:
        lms[l]["observers"].sort()
    for k, l in m["forget_kp"]:
        kps[int(k)].pop(int(l), None)
    for l in m["forget_lm"]:
        lms.pop(int(l), None)
    return poses, kps, lms
