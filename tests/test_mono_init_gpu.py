"""GPU tests of the two mono host stages that use the refined 5-point model (C++ host mirror over its C hooks) against their
numpy restatement tests/mono_init_ref.py: the mono do_optimize branch of VisualFrontEnd::epipolar2d2dFiltering and
VisualFrontEnd::checkReadyForInit.  The maps are those of tests/mono_init_cases.py (tests/test_mono_init_ref_cpu.py checks
the branches they take and their tameness)."""
import numpy as np
import pytest

import mono_init_cases as MC
import relpose_ref as RR
from ov2slam_amd import host_map, synth_epi
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

pytestmark = pytest.mark.gpu


def _map(c):
    m = host_map.MonoMap(c["sc"]["K"], c["poses"])
    for kfid, fr in ((m.nkf - 2, c["kf"]), (m.nkf - 1, c["cur"])):
        for lmid, (px, is3d) in sorted(fr.items()):
            m.add_keypoint(kfid, lmid, px, is3d)
    return m


def _same_pose(T, E, tol=1e-9):
    s = 1.0 if np.dot(T[3:], E[3:]) >= 0 else -1.0       # q and -q are one rotation
    return np.abs(T[:3] - E[:3]).max() < tol and np.abs(s * T[3:] - E[3:]).max() < tol


# ---- mono epipolar2d2dFiltering -----------------------------------------------------------------------------------------
def test_mono_epipolar_uses_the_refined_motion(ctx):
    """three keyframes, fewer than 30 3D keypoints: OV2_OK (not OV2_ERR_UNSUPPORTED), the RANSAC outliers removed, the pose
    set from the refined model with the scale of the motion model"""
    c = MC.epipolar_case(20)
    e = MC.epipolar_ref(c)
    m = _map(c)
    try:
        got, st = m.epipolar_filtering(ctx, MC.NRANSAC, MC.ERRTH, seed=c["seed"])     # raises on a negative status
        T = m.pose()
    finally:
        m.close()
    assert st["status"] == e["status"] == 2 and st["do_optimize"] == 1
    assert (st["refine_status"], st["refine_iters"]) == (e["refine"]["status"], e["refine"]["iters"]) and st["refine_status"] == 1
    assert got.tolist() == e["removed"] and st["removed"] == len(e["removed"]) > 0
    assert _same_pose(T, e["Twc"])
    assert not _same_pose(T, c["poses"][-1], 1e-3)


def test_mono_epipolar_with_30_3d_keypoints_keeps_the_pose(ctx):
    c = MC.epipolar_case(30)
    e = MC.epipolar_ref(c)
    m = _map(c)
    try:
        got, st = m.epipolar_filtering(ctx, MC.NRANSAC, MC.ERRTH, seed=c["seed"])
        T = m.pose()
    finally:
        m.close()
    assert st["status"] == 2 and st["do_optimize"] == 0 and st["refine_status"] == 0 and st["refine_iters"] == 0
    assert got.tolist() == e["removed"]
    assert T.tobytes() == c["poses"][-1].tobytes()


# ---- checkReadyForInit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small_baseline", "seven_shared"])
def test_not_ready(ctx, kind):
    c = MC.init_case(kind)
    assert not MC.init_ref(c)["ready"]
    m = _map(c)
    try:
        ready, removed, st = m.check_ready_for_init(ctx, MC.FINIT, MC.NRANSAC, MC.ERRTH, seed=c["seed"])
        T = m.pose()
    finally:
        m.close()
    assert not ready and len(removed) == 0 and T.tobytes() == c["poses"][-1].tobytes()
    assert st["do_optimize"] == 0 and st["refine_iters"] == 0      # returned before the 5-point call


def test_ready_for_init(ctx):
    c = MC.init_case("n300")
    e = MC.init_ref(c)
    m = _map(c)
    try:
        ready, removed, st = m.check_ready_for_init(ctx, MC.FINIT, MC.NRANSAC, MC.ERRTH, seed=c["seed"])
        T = m.pose()
    finally:
        m.close()
    assert ready and e["ready"]
    assert st["do_optimize"] == 1 and (st["refine_status"], st["refine_iters"]) == (e["refine"]["status"], e["refine"]["iters"])
    assert removed.tolist() == e["removed"] and len(removed) > 0
    assert abs(np.linalg.norm(T[:3]) - 0.25) < 1e-15
    assert _same_pose(T, e["Twc"])
    assert RR.dir_err_deg(T[:3], c["sc"]["t"]) < 1.0


# ---- the refined form by its own name; the old wrappers still refuse ------------------------------------------------------
def test_opt_wrappers_agree_and_old_wrappers_refuse(ctx):
    s = synth_epi.make_scene(300, seed=250, noise_px=0.5, outlier_frac=0.2, baseline=0.5)
    K = s["K"]
    mvg = MultiViewGeometry(ctx)
    ok, R, t, idx, refined = mvg.compute5ptEssentialMatrix_opt(s["bv_kf"], s["bv_cur"], 100, 3.0, True, np.float32(K[0]),
                                                              np.float32(K[1]), seed=5)
    ok2, R2, t2, idx2, ref2 = host_map.compute5pt_essential_opt(ctx, s["bv_kf"], s["bv_cur"], 100, 3.0, K[0], K[1], 5)
    assert ok and ok2 and refined == ref2[0] == 1 and ref2[1] > 0
    assert idx.tolist() == idx2.tolist() and R.tobytes() == R2.tobytes() and t.tobytes() == t2.tobytes()
    with pytest.raises(NotImplementedError):
        mvg.compute5ptEssentialMatrix(s["bv_kf"], s["bv_cur"], 100, 3.0, True, True, K[0], K[1])
    with pytest.raises(RuntimeError):
        host_map.compute5pt_essential(ctx, s["bv_kf"], s["bv_cur"], 100, 3.0, True, K[0], K[1], 1)
