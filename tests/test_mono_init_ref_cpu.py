"""CPU tests of tests/mono_init_ref.py, the numpy restatement of the two mono host stages that use the refined 5-point
model, on the maps of tests/test_mono_init_gpu.py: the branches they are meant to take, and tameness of the refinement where
the GPU test compares poses (the GPU RANSAC's model agrees with the checker's to 1e-8, the bar of tests/test_epipolar_gpu.py,
so the start of the refinement is moved by that much here)."""
import numpy as np
import pytest

import mono_init_cases as MC
import mono_init_ref as MR
import relpose_ref as RR


def test_se3_pieces():
    rng = np.random.default_rng(0)
    q = rng.normal(size=4)
    A = np.concatenate([rng.normal(size=3), q / np.linalg.norm(q)])
    q = rng.normal(size=4)
    B = np.concatenate([rng.normal(size=3), q / np.linalg.norm(q)])
    I = MR.se3_mul(A, MR.se3_inv(A))
    assert np.abs(I[:3]).max() < 1e-15 and np.abs(np.abs(I[6]) - 1) < 1e-15
    AB = MR.se3_mul(A, B)
    x = rng.normal(size=3)
    assert np.abs(MR.se3_R(AB) @ x + AB[:3] - (MR.se3_R(A) @ (MR.se3_R(B) @ x + B[:3]) + A[:3])).max() < 1e-14


def test_epipolar_branches():
    c = MC.epipolar_case(20)
    r = MC.epipolar_ref(c)
    assert r["status"] == 2 and r["do_optimize"] == 1 and r["refine"]["status"] == 1 and len(r["removed"]) > 20
    # the pose moved: scale kept, direction and rotation now the refined model's
    Tk = MR.se3_mul(MR.se3_inv(c["poses"][-2]), r["Twc"])
    T0 = MR.se3_mul(MR.se3_inv(c["poses"][-2]), c["poses"][-1])
    assert abs(np.linalg.norm(Tk[:3]) - np.linalg.norm(T0[:3])) < 1e-12
    sc = c["sc"]
    assert RR.dir_err_deg(Tk[:3], sc["t"]) < 1.0 < RR.dir_err_deg(T0[:3], sc["t"])
    assert RR.rot_err_deg(MR.se3_R(Tk), sc["R"]) < 0.3 < RR.rot_err_deg(MR.se3_R(T0), sc["R"])
    c30 = MC.epipolar_case(30)
    r30 = MC.epipolar_ref(c30)
    assert r30["status"] == 2 and r30["do_optimize"] == 0 and r30["refine"] is None
    assert r30["Twc"].tobytes() == c30["poses"][-1].tobytes() and r30["removed"] == r["removed"]


def test_init_branches():
    for kind, ready in [("n300", True), ("small_baseline", False), ("seven_shared", False)]:
        c = MC.init_case(kind)
        r = MC.init_ref(c)
        assert r["ready"] == ready, kind
        if ready:
            assert abs(np.linalg.norm(r["Twc"][:3]) - 0.25) < 1e-15 and r["refine"]["status"] == 1
            assert len(r["removed"]) >= int(0.15 * len(c["kf"]))
        else:
            assert r["Twc"].tobytes() == c["poses"][-1].tobytes() and not r["removed"]
    assert MC.init_ref(MC.init_case("seven_shared"))["pairs"] == 7          # past the first parallax test, stopped at < 8
    assert MC.init_ref(MC.init_case("small_baseline"))["pairs"] == 0        # stopped at the first parallax test
    r = MC.init_ref(MC.init_case("n300"))
    assert RR.dir_err_deg(r["Twc"][:3], MC.init_case("n300")["sc"]["t"]) < 1.0


def _signature(r):
    return (r["status"], r["iters"], r["term"], tuple(l[1] for l in r["log"]))


@pytest.mark.parametrize("which", ["epipolar", "n300"])
def test_host_scenes_are_tame(which):
    """the refinement of every map whose pose the GPU test compares, started from the RANSAC model moved by up to 1e-8 and
    with bearings moved by up to 1e-13: the same iteration log, and a pose within 1e-10"""
    if which == "epipolar":
        c = MC.epipolar_case(20)
        K = c["sc"]["K"]
    else:
        c = MC.init_case(which)
        K = np.array([float(np.float32(c["sc"]["K"][0])), float(np.float32(c["sc"]["K"][1])), 0., 0.])
    ids, bkf, bcur = MR._pairs(c["kf"], c["cur"], c["sc"]["K"])
    e, R, t, base = MR.ransac_then_refine(bkf, bcur, K, MC.NRANSAC, MC.ERRTH, c["seed"])
    assert base["status"] == 1
    for k in range(3):
        rng = np.random.default_rng(k)
        r = RR.refine(bkf + rng.uniform(-1e-13, 1e-13, bkf.shape), bcur + rng.uniform(-1e-13, 1e-13, bcur.shape), K,
                      e["R"] + rng.uniform(-1e-8, 1e-8, 9), e["t"] + rng.uniform(-1e-8, 1e-8, 3), MR.NREFINE, e["outlier"])
        assert _signature(r) == _signature(base)
        assert np.abs(r["R"] - base["R"]).max() < 1e-10 and np.abs(r["t"] - base["t"]).max() < 1e-10
