"""Cases of the structure-only BA on the map mirrors: windows of synth_ba.make_window(..., inv_depth=False) with their pixels
rounded through float32 (keypoints are cv::Point2f in the map, as tests/test_host_adapter.py::test_structure_only_ba has
them), a non-zero pyramid level on part of the rows, and the listed points moved by seeded Gaussian noise.  A case is a
dict; tables_of(case) is the numpy model of the tables DeviceMap.download() returns for it (the GPU tests check the model
against the download), mirror_of(ctx, case) the mirror itself, built through DeviceMap.from_problem and the public hooks.

Shapes, the smallest at which each piece can go wrong: (10, 400, seed 29) every second id -- 3372 blocks, 3-20 per point,
several workgroups of rows; (40, 60, max_obs 40, random) -- 9-80 blocks per point, up to 40 rows: three chunks of a 16-lane
group; (3, 8) -- fewer points than a wave; (10, 2600) every second id -- 1300 points, more than the workgroup's threads and
than one 1024-wide scan block; `thin` -- the first shape with ten points cut down to one mono row and ten to one stereo
row (2 x 3 jacobians that only the LM diagonal makes solvable); `mono` -- left blocks only.
Branches: FTOL (the first shape), MAX_ITER (max_iters = 3 where five log entries are needed), max_iters 0 and 1, and a log
with rejected steps (`rejected`: noise 2 m on the smallest window; ten iterations do not converge it, and its 1e-13 copies
still agree to 1e-13, so its points are compared like the others)."""
import functools

import numpy as np

from ov2slam_amd import device_map as DM, synth_ba

NOISE_SEED = 4711


def _window(kw):
    P = synth_ba.make_window(inv_depth=False, **kw)
    P.res_uv = P.res_uv.astype(np.float32).astype(np.float64)
    return P


def _case(name, kw, step, noise, max_iters=10, thin=False, term=None, noise_seed=NOISE_SEED, rejected=False):
    return dict(name=name, kw=kw, step=step, noise=noise, max_iters=max_iters, thin=thin, term=term, noise_seed=noise_seed,
                rejected=rejected)


W29 = dict(n_kf=10, n_lm=400, seed=29)
CASES = {c["name"]: c for c in [
    _case("w10x400", W29, 2, 0.1, term="function_tolerance"),
    _case("w40x60", dict(n_kf=40, n_lm=60, max_obs=40, obs_pick="random"), 1, 0.05),
    _case("w3x8", dict(n_kf=3, n_lm=8), 1, 0.05),
    _case("w10x2600", dict(n_kf=10, n_lm=2600), 2, 0.05),
    _case("thin", W29, 2, 0.02, thin=True),
    _case("mono", dict(n_kf=10, n_lm=400, seed=29, stereo=False), 2, 0.1),
    _case("maxiter3", W29, 2, 0.1, max_iters=3, term="max_iter"),
    _case("iters0", W29, 2, 0.1, max_iters=0, term="max_iter"),
    _case("iters1", W29, 2, 0.1, max_iters=1, term="max_iter"),
    _case("rejected", dict(n_kf=3, n_lm=8), 1, 2.0, term="max_iter", noise_seed=1, rejected=True),
]}
SHAPES = ["w10x400", "w40x60", "w3x8", "w10x2600", "thin", "mono"]
BRANCHES = ["maxiter3", "iters0", "iters1", "rejected"]


@functools.lru_cache(maxsize=None)
def problem_of(name):
    """(BaProblem, per-observation scale in the order of DeviceMap.observations_of, listed ids, noisy points of the ids,
    rows to remove as (kfid, lmid), rows whose stereo flag is cleared as (kfid, lmid))"""
    c = CASES[name]
    P = _window(dict(c["kw"]))
    kf, lm, un, st, run = DM.observations_of(P)
    i = np.arange(len(kf))
    scale = np.where(i % 5 == 0, 1, np.where(i % 11 == 0, 2, 0)).astype(np.int32)
    ids = np.arange(len(P.lm), dtype=np.int32)[::c["step"]]
    rng = np.random.default_rng(c["noise_seed"])
    xyz = DM.world_points_of(P)[ids] + rng.normal(0, c["noise"], (len(ids), 3))
    rm, mono = [], []
    if c["thin"]:
        for n, l in enumerate(ids[:20]):
            rows = np.flatnonzero(lm == l)
            keep = rows[np.flatnonzero(st[rows])[0]] if n >= 10 else rows[0]   # a stereo row for the second ten
            rm += [(int(kf[r]), int(l)) for r in rows if r != keep]
            if n < 10:
                mono.append((int(kf[keep]), int(l)))
    return P, scale, ids, xyz, rm, mono


def tables_of(name, noisy=True):
    """the tables of the case's mirror as DeviceMap.download() returns them (spare capacity of from_problem included; slots
    that hold nothing are zero here and unwritten there), and the scale column"""
    P, scale, ids, xyz, rm, mono = problem_of(name)
    kf, lm, un, st, run = DM.observations_of(P)
    nk, nl = len(P.pose), len(P.lm)
    d = dict(kf_pose=np.zeros((nk + 8, 7)), kf_state=np.zeros(nk + 8, np.uint8), lm_xyz=np.zeros((nl + 8, 3)),
             lm_state=np.zeros(nl + 8, np.uint8), obs_kf=kf.copy(), obs_lm=lm.copy(),
             obs_flag=(DM.OBS_ALIVE | np.where(st != 0, DM.OBS_STEREO, 0)).astype(np.uint8), obs_uv=un.copy(), obs_ruv=run.copy())
    d["kf_pose"][:nk], d["kf_state"][:nk] = P.pose, 1
    d["lm_xyz"][:nl] = DM.world_points_of(P)
    d["lm_state"][:nl] = DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D
    d["lm_state"][lm[kf == nk - 1]] |= DM.LM_OBS
    for k, l in rm:
        d["obs_flag"][(kf == k) & (lm == l)] = 0
    for k, l in mono:
        d["obs_flag"][(kf == k) & (lm == l)] &= ~np.uint8(DM.OBS_STEREO)
    if noisy:
        d["lm_xyz"][ids] = xyz
    return d, scale


def cam_of(name):
    P = problem_of(name)[0]
    return P.calib_l, P.calib_r, P.T_rl


def mirror_of(ctx, name, noisy=True):
    """the case's mirror through the public hooks: from_problem, remove_obs, the stereo flags, set_landmarks"""
    import ctypes as C
    P, scale, ids, xyz, rm, mono = problem_of(name)
    dm = DM.DeviceMap.from_problem(ctx, P, scale=scale)
    if rm:
        dm.remove_obs([k for k, _ in rm], [l for _, l in rm])
    if mono:
        k, l = np.array([k for k, _ in mono], np.int32), np.array([l for _, l in mono], np.int32)
        off, ruv = np.zeros(len(k), np.uint8), np.zeros((len(k), 2))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx.lib.ov2_map_set_obs_stereo(dm.h, len(k), vp(k), vp(l), vp(off), vp(ruv)) == 0
    if noisy:
        dm.set_landmarks(ids, xyz, tables_of(name)[0]["lm_state"][ids])
    return dm
