"""What follows an accepted loop (LoopCloser::closeLoop / closeLoops, reference src/loop_closer.cpp:302-372) on the scenes of
ov2slam_amd/synth_close.py: the chain against its steps called one by one on a second copy of the map (bitwise), its decisions
against tests/loop_close_ref.py, the refused and gated branches, the batch of four maps against four single calls, and the
close_loops_ switch of LoopCloser::newKeyframe."""
import numpy as np
import pytest

import loop_close_ref as R
from ov2slam_amd import host_map, lcd, synth_close, synth_revisit

pytestmark = pytest.mark.gpu
NEWKF, LC, INIKF, LOOSE_START = synth_close.NEWKF, synth_close.LC, synth_close.INIKF, synth_close.LOOSE_START
LV_ACCEPTED = 4
H = host_map


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


_scenes = {}


def scene(seed, variant):
    if (seed, variant) not in _scenes:
        _scenes[(seed, variant)] = synth_close.make_scene(seed, variant)
    return _scenes[(seed, variant)]


def verified_map(ctx, s):
    """a fresh host map of the scene with verifyLoopCandidate run on it (it may clear is3d_ of bad map points, so every copy
    that is compared goes through it), and what it returned: the loop pose and the pair list the chain starts from"""
    m = H.LoopMap(s)
    newkf, lckf, pairs = synth_revisit.verify_pairs(s)["accept"]
    v = m.loop_verify_candidate(ctx, newkf, lckf, pairs, 5, nransac_iter=synth_revisit.NRANSAC_ITER, fransac_err=synth_revisit.FRANSAC_ERR)
    assert v["branch"] == LV_ACCEPTED and len(v["final"]) >= 30
    return m, v["Twc"], v["final"]


def state(m, s):
    """every keyframe pose, every landmark and every keyframe's keypoint list, doubles as bit patterns"""
    lmids = sorted(set(int(l) for k in s["kfids"] for l in s["kps"][k]["lmid"]))
    lms = {}
    for l in lmids:
        x, n = m.landmark(l)
        lms[l] = None if x is None else (x.view(np.uint64).tolist(), n)
    return ({k: m.pose(k).view(np.uint64).tolist() for k in s["kfids"]}, lms, m.order())


def result(r):
    """a loop_close dict without the call's counters"""
    return {k: v for k, v in r.items() if k != "last_close"}


def test_big_chain_equals_its_steps(ctx):
    s = scene(1, "big")
    A, Twc, pairs = verified_map(ctx, s)
    B, TwcB, pairsB = verified_map(ctx, s)
    try:
        assert np.array_equal(Twc, TwcB) and pairs == pairsB and state(A, s) == state(B, s)
        stored = B.pose(NEWKF)
        r = A.loop_close(ctx, NEWKF, LC, Twc, pairs)
        # the same steps from Python
        ok, _, nlog = B.local_pose_graph(ctx, NEWKF, INIKF, Twc)
        assert ok == 1 and nlog == r["pg_n_log"]
        moved = np.linalg.norm(B.pose(NEWKF)[:3] - Twc[:3])
        print(f"[loop_close big] new keyframe {np.linalg.norm(stored[:3] - Twc[:3]):.3f} m -> {moved:.3f} m from the loop pose; {r}")
        assert moved < 0.5 * np.linalg.norm(stored[:3] - Twc[:3])
        merged = []
        for prev, new in pairs:
            if prev != new:
                B.merge_points(prev, new)
                merged.append(new)
        after_merge = B.order()      # before the two BAs, which may drop an observation they flag
        for prev, new in pairs:
            if prev != new:
                assert all(prev not in o for o in after_merge.values()) and new in after_merge[NEWKF], (prev, new)
        sba = B.structure_only_ba(ctx, merged)
        loose = B.loose_ba(ctx, LOOSE_START, NEWKF, True)
        assert (r["pg_status"], r["sba_status"], r["loose_status"]) == (0, sba[0], loose[0]) == (0, 0, 0)
        assert state(A, s) == state(B, s)
        # the decisions against the checker
        d = R.decide(len(pairs), [k for k in synth_revisit.COV_OF_LC], LC, stored, Twc, pairs, True, covis_of_inikf=[LOOSE_START])
        assert r["branch"] == d["branch"] == R.LCL_CLOSED_LOOSE_BA == H.LCL_CLOSED_LOOSE_BA
        assert r["inikfid"] == d["inikfid"] == 10 and r["loose_start"] == d["loose_start"] == LOOSE_START
        assert abs(r["lc_pose_err"] - d["lc_pose_err"]) <= 1e-12 and r["lc_pose_err"] >= 0.02
        assert r["merged"] == d["merged"] == merged and len(merged) >= 27
        assert r["last_close"] == dict(jobs=1, graphs=1, solve_calls=1)
        order = A.order()
        for prev, new in pairs:
            if prev == new:
                continue
            assert all(prev not in o for o in order.values()) and A.landmark(prev)[0] is None, prev
    finally:
        A.close()
        B.close()


def test_small_no_loose_ba(ctx):
    s = scene(1, "small")
    A, Twc, pairs = verified_map(ctx, s)
    try:
        stored = A.pose(NEWKF)
        r = A.loop_close(ctx, NEWKF, LC, Twc, pairs)
        print(f"[loop_close small] {r}")
        assert r["branch"] == H.LCL_CLOSED == R.decide(len(pairs), list(synth_revisit.COV_OF_LC), LC, stored, Twc, pairs, True)["branch"]
        assert r["lc_pose_err"] < 0.02 and (r["pg_status"], r["sba_status"]) == (0, 0)
        assert r["loose_status"] == H.LCL_NOT_CALLED and r["loose_start"] == -1      # looseBA was not called: its fields are untouched
    finally:
        A.close()


def test_far_is_refused_and_few_pairs_gated(ctx):
    s = scene(1, "big")
    A, Twc, pairs = verified_map(ctx, s)
    try:
        before = state(A, s)
        r = A.loop_close(ctx, NEWKF, LC, synth_close.far_pose(s), pairs)
        assert r["branch"] == H.LCL_PG_REFUSED and r["pg_status"] == 0 and r["merged"] == []
        assert (r["sba_status"], r["loose_status"]) == (H.LCL_NOT_CALLED, H.LCL_NOT_CALLED)
        assert r["last_close"] == dict(jobs=1, graphs=1, solve_calls=1)     # solved, then refused by the degenerate test
        assert state(A, s) == before
        f = A.loop_close(ctx, NEWKF, LC, Twc, pairs[:29])
        assert f["branch"] == H.LCL_FEW_PAIRS == R.decide(29, list(synth_revisit.COV_OF_LC), LC, A.pose(NEWKF), Twc, pairs[:29], True)["branch"]
        assert f["last_close"] == dict(jobs=1, graphs=0, solve_calls=0) and f["pg_status"] == H.LCL_NOT_CALLED   # no library call
        assert state(A, s) == before
    finally:
        A.close()


def test_batch_of_four_equals_four_single_calls(ctx):
    """big at seeds 1 and 2, small, far.  last_close_ shows ONE solve call and FOUR graphs offered: the far graph has a chain
    and is solved with the others; it is the degenerate test behind the solve that refuses it"""
    cases = [(1, "big", False), (2, "big", False), (1, "small", False), (1, "big", True)]
    maps, singles, args = [], [], []
    try:
        for seed, variant, far in cases:
            s = scene(seed, variant)
            m, Twc, pairs = verified_map(ctx, s)
            one, Twc1, pairs1 = verified_map(ctx, s)
            T = synth_close.far_pose(s) if far else Twc
            singles.append((one.loop_close(ctx, NEWKF, LC, T, pairs1), state(one, s)))
            one.close()
            maps.append(m)
            args.append((T, pairs))
        res = H.loop_close_batch(ctx, maps, [NEWKF] * 4, [LC] * 4, [a[0] for a in args], [a[1] for a in args])
        assert [r["branch"] for r in res] == [H.LCL_CLOSED_LOOSE_BA, H.LCL_CLOSED_LOOSE_BA, H.LCL_CLOSED, H.LCL_PG_REFUSED]
        for (seed, variant, far), m, r, (r1, st1) in zip(cases, maps, res, singles):
            assert result(r) == result(r1), (seed, variant, far)
            assert state(m, scene(seed, variant)) == st1, (seed, variant, far)
            assert r["last_close"] == dict(jobs=4, graphs=4, solve_calls=1)
    finally:
        for m in maps:
            m.close()


def test_close_loops_switch_on_the_revisit_stream(ctx):
    """ov2h_loop_new_keyframe on the synth_loop revisit stream (keyframe 40 proposes keyframe 2).  That scene carries no world
    points, so its candidate does not end LV_ACCEPTED: with the switch on `closed` stays untouched and nothing is solved; with
    it off every field equals the run with it on.  The chain itself is covered by the tests above."""
    from test_lcd_gpu import LC_PARAMS, revisit_map
    runs = []
    for on in (False, True):
        s, m = revisit_map()
        lc = lcd.LoopCloser(ctx, m, **LC_PARAMS)
        try:
            lc.set_close(on)
            out = [lc.new_keyframe(k, 77 + k) for k in s["kfids"] if k <= 40]
            runs.append((out, lc.closed()))
        finally:
            lc.close()
            m.close()
    (off, c_off), (on, c_on) = runs
    assert off == on and off[-1]["cand_kfid"] == 2
    untouched = dict(branch=H.LCL_FEW_PAIRS, inikfid=-1, loose_start=-1, pg_status=H.LCL_NOT_CALLED, sba_status=H.LCL_NOT_CALLED,
                     loose_status=H.LCL_NOT_CALLED, merged=[], pg_termination=0, pg_n_log=0, lc_pose_err=0.0, pg_initial_cost=0.0,
                     pg_final_cost=0.0, last_close=dict(jobs=0, graphs=0, solve_calls=0))
    assert c_off == untouched
    if on[-1]["verify_branch"] == LV_ACCEPTED:
        assert c_on["branch"] >= H.LCL_CLOSED
    else:
        assert c_on == untouched
