"""LoopCloser::trackLoopLocalMap of the C++ host mirror (assembleLoopLocalMap -> ov2_loop_match_to_map_batch -> the pair list)
against the checker (tests/loop_verify_ref.py), EXACTLY: lists in order, every count.  The map's own keypoint order is read
back and handed to the checker; tests/test_loop_verify_ref_cpu.py asserts the gate margins of the same calls on the checker.
LoopCloser::computePnP against the checker over the CPU oracle's ceresPnP.  The whole 2D-3D half (verifyLoopCandidates,
verifyLoopCandidate, processLoopCandidates) on the seven named pairs of synth_revisit.verify_pairs: integers exactly, both poses
within loop_verify_ref.POSE_TOL = 1.0e-7, which tests/test_loop_verify_ref_cpu.py::test_tameness derives on the CPU (10 x the
measured spread of 1.0e-8).  Each case runs in well under a second."""
import numpy as np
import pytest

from ov2slam_amd import host_map, synth_revisit as SR
import loop_verify_ref as LV

pytestmark = pytest.mark.gpu
ARGS = (SR.K4, SR.W, SR.H, SR.CELL, SR.FMAXPROJERR, SR.FDISTRATIO)
KEYS = ("vkplmids", "n_identity", "n_offered", "n_matched")


@pytest.fixture(scope="module")
def world():
    s = SR.make_local_map_scene()
    m = host_map.LoopMap(s)
    order = m.order()
    jobs = SR.track_jobs(s)
    exp = {}
    for name, (newkf, lckf, Twc, pairs) in jobs.items():
        r = LV.track_loop_local_map(s, order, newkf, lckf, pairs, *ARGS, Twc=Twc)
        exp[name] = {k: r[k] for k in KEYS}
    yield s, m, jobs, exp
    m.close()


@pytest.mark.parametrize("name", ["true", "empty_list", "shifted", "away", "other_kf"])
def test_one_pair_against_checker(ctx, world, name):
    s, m, jobs, exp = world
    out, stats = m.loop_track(ctx, [jobs[name]], SR.FMAXPROJERR, SR.FDISTRATIO)
    assert out[0] == exp[name]
    assert stats == dict(pairs=1, match_pairs=1, match_calls=1)


def test_batch_is_single_pairs_in_one_launch(ctx, world):
    s, m, jobs, exp = world
    names = list(jobs) + ["true", "away"]
    out, stats = m.loop_track(ctx, [jobs[n] for n in names], SR.FMAXPROJERR, SR.FDISTRATIO)
    for n, o in zip(names, out):
        assert o == exp[n], n
    assert stats == dict(pairs=len(names), match_pairs=len(names), match_calls=1)
    found = out[0]["vkplmids"][-out[0]["n_matched"]:]
    assert sum(1 for q, l in found if (q, l) in s["true_pairs"]) >= 40                    # the planted revisits are found


def test_pairs_that_do_not_reach_the_matcher(ctx, world):
    s, m, jobs, exp = world
    # keyframe 50's window [35, 65] holds 45, 46, 50 and 60; with every lmid of 45, 46 and 50 as a second element nothing is left to offer
    seconds = sorted(set(int(l) for k in (45, 46, 50) for l in s["kps"][k]["lmid"]))
    job = (SR.NEWKF, 50, s["Twc"], [(SR.NEWKF * 1000 + i, l) for i, l in enumerate(seconds)])
    out, stats = m.loop_track(ctx, [job, jobs["true"]], SR.FMAXPROJERR, SR.FDISTRATIO)
    assert out[0]["n_offered"] == 0 and out[0]["n_matched"] == 0 and out[0]["vkplmids"] == job[3] and out[1] == exp["true"]
    assert stats == dict(pairs=2, match_pairs=1, match_calls=1)
    out, stats = m.loop_track(ctx, [job], SR.FMAXPROJERR, SR.FDISTRATIO)
    assert stats == dict(pairs=1, match_pairs=0, match_calls=0) and out[0]["vkplmids"] == job[3]
    out, stats = m.loop_track(ctx, [])
    assert out == [] and stats == dict(pairs=0, match_pairs=0, match_calls=0)
    with pytest.raises(RuntimeError):
        m.loop_track(ctx, [(SR.NEWKF, 999, s["Twc"], [])])
    with pytest.raises(RuntimeError):                    # keyframe 45 has no keypoint grid
        m.loop_track(ctx, [(45, SR.LC, s["Twc"], [])])


def test_compute_pnp_against_checker(ctx, world, oracle):
    """LoopCloser::computePnP of the host mirror == the checker over the CPU oracle's ceresPnP: the bool, the outlier list
    (given entries first, the appended ones mapped back through vgoodkpidx) exactly, the pose within ceresPnP's own parity band
    of 1e-9 (tests/test_pnp.py); and the true pose is recovered to the scene's noise level -- the checker's own error against
    the truth, x 2"""
    s, m, jobs, exp = world
    pairs, Twc0, out0 = SR.pnp_job(s, exp["true"]["vkplmids"])
    eok, eT, eout, _ = LV.compute_pnp(oracle.pnp_solve, s, SR.NEWKF, pairs, Twc0, SR.K4, out0)
    ok, T, out = m.compute_pnp(ctx, SR.NEWKF, pairs, Twc0, out0)
    assert ok == eok == True and out == eout and len(out) > 10
    assert np.abs(T - eT).max() < 1e-9
    truth = np.asarray(s["Twc"])
    assert np.abs(T[:3] - truth[:3]).max() <= 2 * np.abs(eT[:3] - truth[:3]).max()
    # fewer than three usable pairs: false, pose and list untouched
    ok, T2, out2 = m.compute_pnp(ctx, SR.NEWKF, pairs[:4], Twc0, out0)
    eok2, eT2, eout2, good2 = LV.compute_pnp(oracle.pnp_solve, s, SR.NEWKF, pairs[:4], Twc0, SR.K4, out0)
    assert len(good2) == 2 and ok is False and eok2 is False and out2 == out0 and T2.tobytes() == np.asarray(Twc0).tobytes()


# ---- the whole 2D-3D half: verifyLoopCandidates / verifyLoopCandidate / processLoopCandidates -----------------------------
NAMES = ["accept", "p3p_fail", "gone", "no_new", "pnp_few", "lt4", "outwin"]
EXACT = ("branch", "p3p_status", "p3p_info", "after_p3p", "after_track", "final", "pnp_outliers", "n_identity", "n_offered", "n_matched")


@pytest.fixture(scope="module")
def verify_world(world, oracle):
    s, m, _, _ = world
    order = m.order()
    jobs = SR.verify_pairs(s)
    exp = {n: LV.verify_loop_candidate(oracle.pnp_solve, s, order, *jobs[n], LV.SEED, *ARGS, SR.NRANSAC_ITER, SR.FRANSAC_ERR) for n in NAMES}
    return s, m, jobs, exp


def _same(g, e, name):
    for k in EXACT:
        assert g[k] == e[k], (name, k)
    for k in ("Twc_p3p", "Twc"):                    # tolerance derived on the CPU (loop_verify_ref.POSE_TOL)
        if e[k] is not None:
            assert np.abs(g[k] - e[k]).max() <= LV.POSE_TOL, (name, k, np.abs(g[k] - e[k]).max())
    assert abs(g["lc_pose_err"] - e["lc_pose_err"]) <= 10 * LV.POSE_TOL


def test_verify_all_named_pairs_in_one_call(ctx, verify_world):
    s, m, jobs, exp = verify_world
    out, stats = m.loop_verify(ctx, [jobs[n][:2] for n in NAMES], [jobs[n][2] for n in NAMES], [LV.SEED] * 7, SR.NRANSAC_ITER, SR.FRANSAC_ERR)
    for n, g in zip(NAMES, out):
        _same(g, exp[n], n)
    # one library call per stage whatever B is, each for the pairs that reach it
    assert stats == dict(p3p_pairs=6, refine_pairs=5, track_pairs=5, pnp_pairs=3, p3p_calls=1, refine_calls=1, track_calls=1, pnp_calls=1)
    # accept recovers the TRUE pose to the scene's noise level: the checker's own error against the truth, x 2
    truth = np.asarray(s["Twc"])
    g, e = out[0], exp["accept"]
    assert g["branch"] == LV.LV_ACCEPTED and np.abs(g["Twc"][:3] - truth[:3]).max() <= 2 * np.abs(e["Twc"][:3] - truth[:3]).max()


@pytest.mark.parametrize("name", NAMES)
def test_single_pair_and_reference_shaped_call(ctx, verify_world, name):
    s, m, jobs, exp = verify_world
    out, stats = m.loop_verify(ctx, [jobs[name][:2]], [jobs[name][2]], [LV.SEED], SR.NRANSAC_ITER, SR.FRANSAC_ERR)
    one = m.loop_verify_candidate(ctx, *jobs[name], LV.SEED, SR.NRANSAC_ITER, SR.FRANSAC_ERR)
    _same(out[0], exp[name], name)
    for k in EXACT:
        assert one[k] == out[0][k], k
    assert one["Twc_p3p"].tobytes() == out[0]["Twc_p3p"].tobytes() and one["Twc"].tobytes() == out[0]["Twc"].tobytes()
    assert all(stats[k] <= 1 for k in stats)


def test_refinement_within_the_checkers(ctx, verify_world, oracle):
    """LoopCloser::p3pRansac with do_optimize = true (the stage of verifyLoopCandidate in front of tracking): success, and the pose
    is the checker's RANSAC pose refined by the CPU oracle's ceresPnP on the inliers, not the RANSAC pose itself"""
    s, m, jobs, exp = verify_world
    p = LV.p3p_stage(oracle.pnp_solve, s, SR.NEWKF, jobs["accept"][2], SR.K4, SR.NRANSAC_ITER, SR.FRANSAC_ERR, LV.SEED)
    g = m.loop_verify_candidate(ctx, *jobs["accept"], LV.SEED, SR.NRANSAC_ITER, SR.FRANSAC_ERR)
    assert p["success"] and g["p3p_status"] == 1 and np.abs(g["Twc_p3p"] - p["Twc"]).max() <= LV.POSE_TOL
    assert np.abs(p["Twc"] - p["Twc_ransac"]).max() > 100 * LV.POSE_TOL            # the refinement moved the pose


def test_empty_and_invalid_verify_calls(ctx, verify_world):
    s, m, jobs, exp = verify_world
    out, stats = m.loop_verify(ctx, [], [], [])
    assert out == [] and sum(stats.values()) == 0
    with pytest.raises(RuntimeError):
        m.loop_verify(ctx, [(SR.NEWKF, 999)], [jobs["accept"][2]], [1])
    with pytest.raises(RuntimeError):
        m.loop_verify_candidate(ctx, 999, SR.LC, jobs["accept"][2], 1)


def test_process_is_match_then_verify(ctx):
    """processLoopCandidates on the 2D-2D scene of synth_loop: what matchLoopCandidates gives, then verifyLoopCandidates on the pairs
    that ended LC_PASSED with the lists it passed on"""
    from ov2slam_amd import synth_loop
    s = synth_loop.make_scene()
    m = host_map.LoopMap(s)
    try:
        names = list(s["pairs"])
        pairs, seeds = [s["pairs"][n] for n in names], [1234 + i for i in range(len(names))]
        matched, mstats = m.loop_match(ctx, pairs, seeds)
        br, npass, ver, stats = m.loop_process(ctx, pairs, seeds)
        assert br == [r["branch"] for r in matched] and npass == [len(r["out"]) for r in matched]
        passed = [i for i, r in enumerate(matched) if r["branch"] == 3]              # LC_PASSED
        assert passed
        out, vstats = m.loop_verify(ctx, [(pairs[i][0], matched[i]["lckfid"]) for i in passed], [matched[i]["out"] for i in passed],
                                    [seeds[i] for i in passed])
        for i, g in zip(passed, out):
            for k in EXACT:
                assert ver[i][k] == g[k], k
            assert ver[i]["Twc"].tobytes() == g["Twc"].tobytes()
        for i in set(range(len(pairs))) - set(passed):
            assert ver[i]["p3p_status"] == -1 and ver[i]["after_p3p"] == []
        assert {k: stats[k] for k in mstats} == mstats and {k: stats[k] for k in vstats} == vstats
    finally:
        m.close()
