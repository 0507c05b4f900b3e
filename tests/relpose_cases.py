"""the scenes of tests/test_relpose_gpu.py, shared with the tameness test of tests/test_relpose_ref_cpu.py: built once, the
checker's results computed once and left unchanged."""
import functools

import numpy as np

import relpose_ref as RR
from ov2slam_amd import synth_ba, synth_epi

MAX_ITERS = 10
# admitted pairs per frame: below the minimum, the minimum, wave (64) and workgroup (256) stride edges, several passes
EDGE_N = [0, 5, 6, 10, 63, 64, 65, 255, 256, 257, 2048]
# pairs the skip mask leaves out, per frame (0 = an all-zero mask)
EDGE_SKIPPED = [3, 0, 2, 0, 9, 0, 1, 30, 0, 5, 300]
# scene seed per frame: chosen so that every frame is tame (test_relpose_ref_cpu.test_gpu_scenes_are_tame)
EDGE_SEED = [200, 201, 202, 203, 204, 205, 206, 207, 208, 209, 210]


def perturbed(R, t, rot_deg, dir_deg, seed):
    """ground truth moved by rot_deg about a seeded axis and by dir_deg in the direction of t"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    dR, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), np.deg2rad(rot_deg) * a]))
    p = np.cross(t, rng.normal(size=3))
    p /= np.linalg.norm(p)
    tp = np.cos(np.deg2rad(dir_deg)) * t + np.sin(np.deg2rad(dir_deg)) * p
    return dR @ R, tp / np.linalg.norm(tp)


def make_case(n_adm, n_skip, seed, rot_deg=1.0, dir_deg=5.0):
    """n_adm admitted pairs of a 0.5 px scene and n_skip skipped pairs with unrelated bearings, interleaved by a seeded
    permutation; the start is the perturbed truth.  skip is None where n_skip = 0."""
    n = n_adm + n_skip
    s = synth_epi.make_scene(max(n, 1), seed=seed, noise_px=0.5, outlier_frac=0.0)
    rng = np.random.default_rng(1000 + seed)
    f1, f2 = s["bv_kf"][:n].copy(), s["bv_cur"][:n].copy()
    skip = np.zeros(n, np.uint8)
    if n_skip:
        bad = rng.permutation(n)[:n_skip]
        skip[bad] = 1
        v = rng.normal(size=(n_skip, 3))
        f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    R0, t0 = perturbed(s["R"], s["t"], rot_deg, dir_deg, seed)
    return dict(f1=f1, f2=f2, skip=skip if n_skip else None, K=s["K"], R0=R0.reshape(9), t0=t0, Rgt=s["R"], tgt=s["t"])


@functools.lru_cache(maxsize=None)
def edge_batch():
    return [make_case(n, k, sd) for n, k, sd in zip(EDGE_N, EDGE_SKIPPED, EDGE_SEED)]


def exact_case(n=40, seed=5):
    """bearings that satisfy the epipolar constraint exactly in floating point: R = I, t = e_x, integer points, bearings
    left unnormalised (the cost is defined for any bearing): every residual is an exact 0"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.integers(-8, 9, n), rng.integers(-8, 9, n), rng.integers(3, 12, n)], 1).astype(np.float64)
    t = np.array([1.0, 0, 0])
    return dict(f1=X, f2=X - t, skip=None, K=synth_epi.K_EUROC, R0=np.eye(3).reshape(9), t0=t, Rgt=np.eye(3), tgt=t)


def nan_case(seed=220):
    c = make_case(100, 0, seed)
    c["f2"][37, 1] = np.nan
    return c


@functools.lru_cache(maxsize=None)
def refusal_batch():
    """a good frame, the exact frame, a good frame, the NaN frame, a good frame"""
    return [make_case(120, 0, 221), exact_case(), make_case(70, 4, 222), nan_case(), make_case(300, 10, 223)]


@functools.lru_cache(maxsize=None)
def chain_scenes():
    """RANSAC + refinement chain: status 2, status 2, too few pairs (status 0), too many outliers (status 1)"""
    return [synth_epi.make_scene(300, seed=230, noise_px=0.5, outlier_frac=0.2),
            synth_epi.make_scene(64, seed=231, noise_px=0.5, outlier_frac=0.2),
            synth_epi.make_scene(7, seed=232, outlier_frac=0.0),
            synth_epi.make_scene(200, seed=233, outlier_frac=0.55, baseline=0.5)]


def run_ref(c, max_iters=MAX_ITERS, eps=0.0, seed=0):
    """the checker on a case, its inputs optionally perturbed by eps (uniform, every bearing / R / t entry)"""
    f1, f2, R0, t0 = c["f1"], c["f2"], c["R0"], c["t0"]
    if eps:
        rng = np.random.default_rng(seed)
        f1 = f1 + rng.uniform(-eps, eps, f1.shape)
        f2 = f2 + rng.uniform(-eps, eps, f2.shape)
        R0 = R0 + rng.uniform(-eps, eps, R0.shape)
        t0 = t0 + rng.uniform(-eps, eps, t0.shape)
    return RR.refine(f1, f2, c["K"], R0, t0, max_iters, c["skip"])


@functools.lru_cache(maxsize=None)
def edge_refs():
    return [run_ref(c) for c in edge_batch()]


@functools.lru_cache(maxsize=None)
def refusal_refs():
    return [run_ref(c) for c in refusal_batch()]


def all_gpu_cases():
    """every frame the GPU tests compare against the checker, but the exact frame: its sums are exact zeros in any order
    (integers), and moving its inputs would take away the one property it is there for"""
    return edge_batch() + [c for i, c in enumerate(refusal_batch()) if i != 1]
