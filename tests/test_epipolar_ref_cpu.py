"""CPU checks of the numpy restatement of the per-frame epipolar filter (tests/epipolar_ref.py), the checker that
tests/test_epipolar_gpu.py compares the kernel against: its 5-point solver, its RANSAC, the sampler and the threshold."""
import numpy as np

import epipolar_ref as ER
from ov2slam_amd import synth_epi


def _near(E, Eg, tol):
    return min(np.abs(E - Eg).max(), np.abs(E + Eg).max()) < tol


def test_solver_returns_ground_truth():
    bv1, bv2, Eg = synth_epi.random_samples(200, seed=3)
    for i in range(200):
        sols = ER.fivept_stewenius(bv1[i], bv2[i])
        assert 1 <= len(sols) <= 10 and len(sols) % 2 == 0
        assert any(_near(E.reshape(3, 3), Eg[i], 1e-9) for E in sols), i
        for E in sols:
            E = E.reshape(3, 3)
            assert abs(np.linalg.det(E)) < 1e-8
            assert np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max() < 1e-8
            assert np.abs(np.einsum("ia,ab,ib->i", bv1[i], E, bv2[i])).max() < 1e-8


def test_ransac_recovers_ground_truth_without_outliers():
    for seed in range(3):
        s = synth_epi.make_scene(120, seed=seed, noise_px=0.0, outlier_frac=0.0)
        r = ER.epipolar_filter(s["bv_kf"], s["bv_cur"], s["K"], 100, 3.0, 1000 + seed)
        assert r["status"] == 2 and not r["outlier"].any()
        assert r["info"][3] == 120 and r["info"][1] == 0
        # exact geometry up to the float pixels the bearings are made from
        assert np.abs(r["R"].reshape(3, 3) - s["R"]).max() < 1e-5
        assert np.abs(r["t"] - s["t"]).max() < 1e-4


def test_sampler_distinct_in_range_and_pure():
    for n in (8, 9, 30, 308, 4096):
        for d in range(200):
            idx = ER.draw(77, d, n)
            assert len(set(idx)) == 5 and all(0 <= i < n for i in idx)
            assert idx == ER.draw(77, d, n)
    assert ER.draw(1, 0, 100) != ER.draw(2, 0, 100)
    # one fixed value of the stream, as documented in include/ov2slam_hip.h
    assert ER.draw(12345, 7, 30) == [29, 0, 7, 12, 15]


def test_threshold_value():
    # focal = float(458.654f + 458.654f) / 2, q = 3.f / focal in float, 2 (1 - cos(atan((double)q)))
    th = ER.threshold(3.0, 458.654, 458.654)
    assert th == 4.2781715015483e-05
    # the float overloads of atan / cos would differ in the 4th significant digit at most
    q = np.float32(3.0) / np.float32(458.654)
    thf = 2.0 * (1.0 - float(np.cos(np.arctan(np.float32(q)))))
    assert abs(thf - th) < 3e-3 * th
