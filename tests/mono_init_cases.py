"""the maps of tests/test_mono_init_gpu.py, shared with the CPU tests of their numpy restatement (tests/mono_init_ref.py)."""
import functools

import numpy as np

import mono_init_ref as MR
import relpose_cases as RC
from ov2slam_amd import synth_ba, synth_epi

NRANSAC, ERRTH, FINIT = 100, 3.0, 20.0


def _frames(sc, n3d, n_shared=None, extra_cur=0, seed=0):
    """keyframe / current frame dicts of a scene: the first n3d ids 3D; ids from n_shared on only in the current frame"""
    n = len(sc["unpx_kf"])
    n_shared = n if n_shared is None else n_shared
    kf = {i: (sc["unpx_kf"][i], i < n3d) for i in range(n_shared)}
    cur = {i: (sc["unpx_cur"][i], i < n3d) for i in range(n)}
    rng = np.random.default_rng(seed)
    for j in range(extra_cur):
        cur[5000 + j] = (rng.uniform([20, 20], [730, 460]).astype(np.float32), False)
    return kf, cur


@functools.lru_cache(maxsize=None)
def epipolar_case(n3d):
    """three keyframes and a current frame at a motion-model pose that is off in rotation, direction and scale; n3d of its
    keypoints are 3D (fewer than 30: the do_optimize branch)"""
    sc = synth_epi.make_scene(200, seed=240, noise_px=0.5, outlier_frac=0.2, baseline=0.4)
    T2 = synth_ba.pose7(synth_ba.se3_exp(np.array([0, 0, 0, 0.02, -0.05, 0.03]))[0], np.array([0.4, -0.1, 1.2]))
    Rm, tm = RC.perturbed(sc["R"], sc["t"], 1.5, 10.0, 7)
    T_rel = synth_ba.pose7(Rm, 0.37 * tm)
    poses = [np.array([0, 0, 0, 0, 0, 0, 1.0]), np.array([0.1, 0, 0.5, 0, 0, 0, 1.0]), T2, MR.se3_mul(T2, T_rel)]
    kf, cur = _frames(sc, n3d, extra_cur=6, seed=3)
    return dict(sc=sc, poses=poses, kf=kf, cur=cur, seed=91)


@functools.lru_cache(maxsize=None)
def init_case(kind):
    """two-view mono map: keyframe 0 at identity, the current frame (still at identity: nothing has moved it yet) with the
    scene's pixels"""
    I7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
    if kind == "n300":
        sc = synth_epi.make_scene(300, seed=250, noise_px=0.5, outlier_frac=0.2, baseline=0.5)
        kf, cur = _frames(sc, 0, extra_cur=5, seed=4)
    elif kind == "small_baseline":      # below finit_parallax_
        sc = synth_epi.make_scene(300, seed=252, noise_px=0.5, outlier_frac=0.0, baseline=0.002, rot_deg=0.5)
        kf, cur = _frames(sc, 0)
    elif kind == "seven_shared":        # 7 keypoints shared with the keyframe (of 40 in the current frame)
        sc = synth_epi.make_scene(40, seed=253, noise_px=0.5, outlier_frac=0.0, baseline=0.5)
        kf, cur = _frames(sc, 0, n_shared=7)
    else:
        raise ValueError(kind)
    return dict(sc=sc, poses=[I7, I7.copy()], kf=kf, cur=cur, seed=93)


def epipolar_ref(c):
    return MR.mono_epipolar2d2d(c["kf"], c["cur"], c["sc"]["K"], c["poses"][-2], c["poses"][-1], len(c["poses"]), NRANSAC,
                                ERRTH, c["seed"])


def init_ref(c):
    return MR.check_ready_for_init(c["kf"], c["cur"], c["sc"]["K"], c["poses"][-2], c["poses"][-1], FINIT, NRANSAC, ERRTH,
                                   c["seed"])
