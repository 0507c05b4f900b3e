"""tests/stereo_tri_ref.py (the checker of the stereo-triangulation stage, a restatement of Mapper::triangulateStereo, reference
src/mapper.cpp:346-461) on the maps of ov2slam_amd/synth_stereo_tri.py, without a GPU: the consistent points come back by an
independent route, every branch of the reference is reached, and no keypoint of the maps the GPU tests use stands within 1e-6
of a threshold (so their exclusion rule excludes nothing)."""
import numpy as np
import pytest

from ov2slam_amd import synth_stereo_tri as SST

import stereo_tri_ref as SR


@pytest.fixture(scope="module")
def O():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_py
    return oracle_py


def _run(O, m):
    poses, kps, lms = SST.as_dicts(m)
    return SR.triangulate_stereo(O, poses, kps, lms, m["newkf"], m["K4"], m["Kr"], m["Tlr"], m["rectified"], SR.MAX_REPROJ_ERR), kps


_RESULTS = {}


def _case(O, nk, nl, seed, rectified):
    key = (nk, nl, seed, rectified)
    if key not in _RESULTS:
        m = SST.make_map(nk, nl, seed=seed, rectified=rectified)
        _RESULTS[key] = (m,) + _run(O, m)
    return _RESULTS[key]


def test_rectified_points_equal_depth_from_disparity(O):
    """the disparity form against z = fx b / d in float64: the reference keeps z as a float, one rounding of 2^-24 relative"""
    m, res, kps = _case(O, 4, 1500, 32, True)
    n = 0
    for r in res:
        if m["lm_kind"][r["lmid"]] != "clean":
            continue
        assert r["status"] == SR.OK, r
        kp = kps[m["newkf"]][r["lmid"]]
        X = SR.depth_from_disparity(kp["unpx"], kp["runpx"], m["K4"], SST.BASELINE)
        assert np.abs(r["pt_a"] - X).max() <= 2.0 ** -23 * np.abs(X).max(), (r["pt_a"], X)
        assert abs(r["invdepth"] - 1.0 / r["pt_a"][2]) == 0.0
        n += 1
    assert n > 100


@pytest.mark.parametrize("rectified", [True, False])
def test_consistent_points_lie_near_the_truth(O, rectified):
    """0.3 px of noise on both pixels: the depth moves by z^2 / (fx b) per pixel of disparity, the point sideways by z / fx per
    pixel; six standard deviations of both (disparity noise sqrt(2) * 0.3 px), 10 % on top for the general rig's other
    intrinsics and rotation"""
    m, res, _ = _case(O, 4, 1500, 31, rectified)
    n = 0
    for r in res:
        if m["lm_kind"][r["lmid"]] != "clean":
            continue
        assert r["status"] == SR.OK, r
        z = r["pt_a"][2]
        bound = 1.1 * 6.0 * np.sqrt(2.0) * 0.3 * (z * z / (m["K4"][0] * SST.BASELINE) + z / m["K4"][0])
        assert np.linalg.norm(r["wpt"] - m["lm_xyz"][r["lmid"]]) <= bound, (r, bound)
        n += 1
    assert n > 100


@pytest.mark.parametrize("rectified", [True, False])
@pytest.mark.parametrize("nk,nl,seed", SR.GPU_CASES)
def test_every_branch_is_reached_and_clear_of_the_thresholds(O, nk, nl, seed, rectified):
    """OK, BEHIND, REPROJ and not-selected keypoints in every case; NEG_DISP in every rectified case -- the mid-point method
    has no such exit (:410-425), there a right pixel on the wrong side ends at the depth gate.  And the condition that lets the
    GPU tests compare the verdicts exactly: nothing within 1e-6 of a threshold"""
    m, res, kps = _case(O, nk, nl, seed, rectified)
    seen = {r["status"] for r in res}
    want = {SR.OK, SR.BEHIND, SR.REPROJ} | ({SR.NEG_DISP} if rectified else set())
    assert seen == want, sorted(SR.VERDICT_NAMES[s] for s in want ^ seen)
    new = kps[m["newkf"]]
    assert len(res) < len(new)
    assert any(kp["is3d"] and kp["stereo"] for kp in new.values()) and any(not kp["is3d"] and not kp["stereo"] for kp in new.values())
    # stereo rows of older keyframes on landmarks that are still 2D, dead rows and dead landmarks
    if nk > 1:
        assert any(kp["stereo"] and not kp["is3d"] for k in kps if k != m["newkf"] for kp in kps[k].values())
    assert (m["obs_alive"] == 0).any() and (m["lm_alive"] == 0).any()
    worst = min(r["margin"] for r in res)
    assert worst >= 1e-6, (nk, nl, seed, rectified, worst)
