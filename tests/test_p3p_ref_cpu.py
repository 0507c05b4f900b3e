"""pins tests/p3p_ref.py, the numpy checker of the P3P stage, without a GPU."""
import math

import numpy as np
import pytest

import epipolar_ref as ER
import p3p_ref as PR
from ov2slam_amd import synth_p3p


def _pose_err(r, s):
    return max(np.abs(r["R"].reshape(3, 3) - s["R"]).max(), np.abs(r["t"] - s["t"]).max())


def test_ground_truth_among_solver_roots():
    """Grunert + Procrustes on exact samples: every solution is a rotation that maps the points onto their bearings, the
    ground truth is among them (missing in at most 0.1 % of the samples), 1 to 4 solutions"""
    bv, X, Rg, tg = synth_p3p.random_samples(1500, seed=3)
    missing = 0
    for i in range(len(bv)):
        S = PR.p3p_grunert(bv[i], X[i])
        assert len(S) <= 4
        for R, t in S:
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0
            p = (X[i] - t) @ R
            assert ((p * bv[i]).sum(1) > 0).all()
            assert np.abs(p / np.linalg.norm(p, axis=1, keepdims=True) - bv[i]).max() < 1e-9
        missing += not any(np.abs(R - Rg[i]).max() < 1e-7 and np.abs(t - tg[i]).max() < 1e-7 for R, t in S)
    assert missing <= 0.001 * len(bv)


def test_sampler_is_the_epipolar_stream_cut_after_four():
    for seed, n in [(0, 5), (7, 8), (99, 30), (2 ** 63 + 5, 308), (12345, 4096)]:
        for d in range(40):
            assert PR.draw(seed, d, n) == ER.draw(seed, d, n)[:4]
    for d in range(20):      # n = 4: a permutation of all indices, through the bounded fallback if need be
        assert sorted(PR.draw(3, d, 4)) == [0, 1, 2, 3]


def test_threshold_hand_values():
    th = PR.threshold(3.0, 458., 458.)
    assert th == 1.0 - math.cos(math.atan(float(np.float32(3.0) / np.float32(458.0))))
    assert abs(th - 2.1451e-5) < 1e-8                      # (3 / 458)^2 / 2 to first order
    # no factor 2, unlike the epipolar stage
    assert abs(ER.threshold(3.0, 458., 458.) - 2 * th) < 1e-18
    # float focal: fx + fy rounds in float before the halving
    fx, fy = 458.654, 457.296
    foc = np.float32(np.float64(np.float32(np.float32(fx) + np.float32(fy))) / 2.)
    assert PR.threshold(2.0, fx, fy) == 1.0 - math.cos(math.atan(float(np.float32(np.float32(2.0) / foc))))


def test_distance_rules():
    R, t = np.eye(3).ravel(), np.zeros(3)
    f = np.array([[0, 0, 1.], [0, 0, 1.], [0, 0, 0.], [np.nan, 0, 1.], [0, 0, 1.]])
    X = np.array([[0, 0, 2.], [1, 0, 1.], [0, 0, 2.], [0, 0, 2.], [0, 0, 0.]])
    d = PR.dist(R, t, f, X)
    assert d[0] == 0. and abs(d[1] - (1 - 1 / math.sqrt(2))) < 1e-15
    assert d[2] == 1.0                                   # a zero bearing has distance 1: finite, never an inlier
    assert np.isinf(d[3]) and np.isinf(d[4])             # NaN bearing / point at the camera centre: +infinity
    assert PR.penalty(np.array([4., 0., 1., 9.])) == (1. + 2.) / 2 and PR.penalty(np.array([4., 0., 9.])) == 2.


@pytest.mark.parametrize("n", [6, 9, 30, 308])
@pytest.mark.parametrize("frac", [0.0, 0.2, 0.4])
def test_lmeds_recovers_noise_free_pose(n, frac):
    s = synth_p3p.make_scene(n, seed=10 * n + int(10 * frac), outlier_frac=frac, noise_px=0.0)
    r = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], 100, 3.0, True, seed=n + 1)
    assert r["info"][0] == 100 and r["info"][3] == n - s["outlier"].sum() and _pose_err(r, s) < 1e-8
    if n - s["outlier"].sum() < 5:      # n = 6 at 40 %: the right model, but 4 inliers are the reference's false
        assert r["status"] == 0 and not r["outlier"].any()
    else:
        assert r["status"] == 1 and np.array_equal(r["outlier"], s["outlier"])


def test_lmeds_small_n_terminates():
    for n in (3, 4, 5):
        s = synth_p3p.make_scene(n, seed=n, outlier_frac=0.25, noise_px=0.0)
        r = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], 20, 3.0, True, seed=1)
        assert r["status"] in (0, 1) and r["info"][0] + r["info"][1] <= 11 * 20
        if n < 4:
            assert r["status"] == 0 and r["info"] == [0, 0, -1, 0]


def _ransac_brute(bv, X, nmaxiter, th, seed):
    """OpenGV's loop written out draw by draw, with everything recomputed per draw"""
    n = len(bv)
    it = skipped = d = 0
    k, best, best_d = 1.0, -(2 ** 31 - 1), -1
    while n >= 4 and it < k and skipped < 10 * nmaxiter:
        idx = PR.draw(seed, d, n)
        d += 1
        ok, R, t = PR.model(bv[idx], X[idx])
        if not ok:
            skipped += 1
            continue
        cnt = sum(1 for i in range(n) if PR.dist(R, t, bv[i], X[i])[0] < th)
        if cnt > best:
            best, best_d = cnt, d - 1
            k = math.log(0.01) / math.log(min(max(PR.EPS, 1.0 - (best / n) ** 4.0), 1.0 - PR.EPS))
        it += 1
        if it > nmaxiter:
            break
    return [it, skipped, best_d]


@pytest.mark.parametrize("n,frac,nmaxiter", [(30, 0.2, 100), (120, 0.4, 100), (60, 0.0, 1), (40, 0.5, 5)])
def test_ransac_equals_brute_force_loop(n, frac, nmaxiter):
    s = synth_p3p.make_scene(n, seed=n, outlier_frac=frac, noise_px=0.3)
    th = PR.threshold(3.0, s["K"][0], s["K"][1])
    r = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], nmaxiter, 3.0, False, seed=5)
    assert r["info"][:3] == _ransac_brute(s["bv"], s["wpts"], nmaxiter, th, 5)
    if frac <= 0.4 and nmaxiter == 100:
        assert r["status"] == 1 and r["outlier"][s["outlier"]].all()
