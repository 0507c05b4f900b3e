"""tests/temporal_ref.py (the checker of the temporal-triangulation stage, a restatement of Mapper::triangulateTemporal,
reference src/mapper.cpp:191-344) on the maps of ov2slam_amd/synth_temporal.py, without a GPU: the geometry comes back
exactly on noise-free pixels, every branch of the reference is reached, the parallax agrees with an independent formula,
and no keypoint of the maps the GPU tests use stands within 1e-6 of a threshold (so their exclusion rule excludes nothing)."""
import numpy as np
import pytest

from ov2slam_amd import synth_temporal

import temporal_ref as TR


@pytest.fixture(scope="module")
def O():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_py
    return oracle_py


def _run(O, m, stereo, exact_px=False):
    poses, kps, lms = synth_temporal.as_dicts(m, exact_px=exact_px)
    return TR.triangulate_temporal(O, poses, kps, lms, m["newkf"], m["K4"], stereo, TR.MAX_REPROJ_ERR), (poses, kps, lms)


def test_noise_free_points_come_back(O):
    """bearings from the exact pixels: the mid-point of two intersecting rays is the point itself (1e-9, the bar of
    test_oracle_tri.py); compared where the generator promises conditioning (baseline >= 5 cm, depth <= 10 m)"""
    m = synth_temporal.make_map(8, 1200, seed=3, noise_px=0.0)
    res, _ = _run(O, m, True, exact_px=True)
    n = 0
    for r in res:
        if r["branch"] != TR.GOOD or m["lm_kind"][r["lmid"]] != "clean" or r["baseline"] < 0.05:
            continue
        assert np.abs(r["wpt"] - m["lm_xyz"][r["lmid"]]).max() < 1e-9
        assert r["pt_a"][2] <= 10.0 and abs(r["invdepth"] - 1.0 / r["pt_a"][2]) == 0.0
        n += 1
    assert n > 100
    # every clean, well-conditioned candidate passed the gates
    clean = [r for r in res if r["branch"] >= TR.GOOD and m["lm_kind"][r["lmid"]] == "clean" and r["baseline"] >= 0.05]
    assert all(r["branch"] == TR.GOOD for r in clean)


def test_every_branch_is_reached(O):
    for nk, nl, seed in ((4, 300, 11), (8, 1500, 12), (12, 4000, 13)):
        m = synth_temporal.make_map(nk, nl, seed=seed)
        on, _ = _run(O, m, True)
        off, _ = _run(O, m, False)
        seen = {r["branch"] for r in on}
        if nl >= 1500:
            assert seen == set(range(12)), sorted(TR.BRANCH_NAMES[b] for b in set(range(12)) - seen)
        # the pair closer than 1 cm: skipped with a stereo rig, candidates without
        nm = [r["lmid"] for r in on if r["branch"] == TR.NO_MOTION]
        assert nm and all(r["kfid"] == m["near_kf"] for r in on if r["branch"] == TR.NO_MOTION)
        by_id = {r["lmid"]: r for r in off}
        assert all(by_id[l]["branch"] in (TR.KP_MISSING,) or by_id[l]["branch"] >= TR.GOOD for l in nm)
        assert TR.NO_MOTION not in {r["branch"] for r in off}
        # everything else takes the same branch with either setting
        assert all(by_id[r["lmid"]]["branch"] == r["branch"] for r in on if r["branch"] != TR.NO_MOTION)
        # outliers of both kinds on either side of 20 px
        for a, b in ((TR.BEHIND_REMOVED, TR.BEHIND_KEPT), (TR.REPROJ_REMOVED, TR.REPROJ_KEPT)):
            if nl >= 1500:
                assert a in seen and b in seen


def test_parallax_against_the_infinite_homography(O):
    m = synth_temporal.make_map(8, 1500, seed=5)
    res, (poses, kps, _) = _run(O, m, False)
    n = 0
    for r in res:
        if r["branch"] < TR.GOOD:
            continue
        p = TR.parallax_independent(poses, r["kfid"], m["newkf"], r["ua"], r["ub"], m["K4"])
        assert abs(p - r["parallax"]) < 1e-3      # the reference rounds the rotated pixel to float
        n += 1
    assert n > 200


@pytest.mark.parametrize("stereo", [True, False])
def test_gpu_maps_keep_clear_of_the_thresholds(O, stereo):
    """the GPU tests compare the gates' verdicts except within 1e-6 (relative) of a threshold: nothing is that close"""
    for nk, nl, seed in TR.GPU_CASES:
        for dangling in (True, False):
            m = synth_temporal.make_map(nk, nl, seed=seed, dangling=dangling)
            res, _ = _run(O, m, stereo)
            worst = min(r["margin"] for r in res)
            assert worst >= 1e-6, (nk, nl, seed, dangling, worst)
