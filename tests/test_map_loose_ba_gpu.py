"""Optimizer::looseBA on the map mirrors (ov2_map_loose_ba_setup_batch / _update_batch / ov2_map_loose_ba_batch,
csrc/map.hip; reference src/optimizer.cpp:900-1672): the set-up against the host walk Optimizer::setupRangeBA, the update
against Optimizer::applyLooseBA on the same crafted state, the whole statement against Optimizer::looseBA, and the batch,
row-order, chain and refusal properties the header states.  Scenes: tests/loose_ba_cases.py (their conditions are asserted
on the CPU in tests/test_loose_ba_ref_cpu.py); the numpy statement: tests/loose_ba_ref.py."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, host_map, synth_close, synth_revisit

import loose_ba_cases as LC
import loose_ba_ref as LR
from test_loose_ba_ref_cpu import SCENES, assert_same_problem

pytestmark = pytest.mark.gpu

INVALID = -1   # OV2_ERR_INVALID (include/ov2slam_hip.h)
TABLES = ("kf_pose", "kf_state", "lm_xyz", "lm_state", "obs_kf", "obs_lm", "obs_flag", "obs_uv", "obs_ruv")

# Whole statement, host form against mirror form: the two solve ONE problem with its rows in two orders.  Measured with the
# CPU oracle (oracle.ba_solve, looseBA's options) on the two orders of every scene used here
# (tests/test_loose_ba_ref_cpu.py::test_whole_statement_scenes_are_well_conditioned prints them):
#   12 kf inverse depth: poses 1.1e-15, points 1.3e-13 relative      12 kf XYZ: 0, 0
#   70 kf inverse depth: poses 4.3e-15, points 9.7e-12 relative      70 kf XYZ: 0, 0
# The tolerance is 100 x the largest spread (the factor covers the GPU solver's own reduction order), capped at 1e-9.
LOOSE_POSE_TOL = 100 * 4.3e-15
LOOSE_POINT_TOL = min(100 * 9.7e-12, 1e-9)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


class _Handle:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.lib, h
    _p = staticmethod(DM.DeviceMap._p)
    download = DM.DeviceMap.download


def same_tables(a, b):
    """byte for byte; slots that hold nothing were never written"""
    if not all(np.array_equal(a[k], b[k]) for k in TABLES if k not in ("kf_pose", "lm_xyz")):
        return False
    kf, lm = a["kf_state"] != 0, (a["lm_state"] & DM.LM_ALIVE) != 0
    return np.array_equal(a["kf_pose"][kf].view(np.uint64), b["kf_pose"][kf].view(np.uint64)) and \
        np.array_equal(a["lm_xyz"][lm].view(np.uint64), b["lm_xyz"][lm].view(np.uint64))


def scene(name, inv_depth, **kw):
    return LC.make_scene(inv_depth=inv_depth, **dict(SCENES[name], **kw))


def adopt_points(dm, hm):
    """the device map takes the host map's landmark points bit for bit (the two constructors round the inverse-depth world
    points differently in the last place); the states must agree already"""
    _, lms, _ = hm.export()
    ids = np.array(sorted(lms), np.int32)
    st = dm.download()["lm_state"][ids]
    assert [int(x) for x in st] == [lms[int(i)][1] for i in ids]
    dm.set_landmarks(ids, np.array([lms[int(i)][0] for i in ids]), st)


def setup_one(ctx, dm, s, stereo=True):
    v = DM.loose_setup_batch(ctx, [dm], [s["ini"]], [s["n"]], 1 if stereo else 2, s["inv_depth"], s["P"].calib_l)
    return v, DM.fetch_view(ctx, v[0], s["inv_depth"])


def assert_ascending(pb):
    assert np.all(np.diff(pb["pose_kfid"]) > 0) and np.all(np.diff(pb["lm_lmid"]) > 0)


# ---- set-up ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", list(SCENES))
def test_setup_equals_the_host_walk(ctx, name, inv_depth, stereo):
    """keyframes with their constness and poses, anchors and anchor pixels, the multiset of residual blocks and the bad list:
    exactly those of Optimizer::setupRangeBA(ini, n, n, 0).  The inverse depth itself is 1 / z with z = R'(p - t) here and
    (Tcw * p).z there: equal to 1e-12 relative, as in tests/test_map_gpu.py"""
    s = scene(name, inv_depth)
    hm = LC.build_host(s, stereo=stereo)
    want = hm.setup_range_ba(s["ini"], s["n"], kf_obs_max=s["n"], min_obs=0)
    dm = LC.build_device(ctx, s)
    try:
        v, got = setup_one(ctx, dm, s, stereo)
        assert not got["aborted"] and not got["outlier"].any()
        assert_same_problem(want, got, inv_depth)
        assert np.array_equal(hm.bad_lmids(), got["bad_lmid"])
        assert_ascending(got)
        if name in ("one", "empty"):
            assert v[0].n_res == 0
        else:
            assert v[0].n_res > 1000
        if name == "removed":   # keyframes 3 and 4 went with ov2_map_remove_keyframe: constness passes to the next live ones
            cst = {int(k) for k, c in zip(got["pose_kfid"], got["pose_const"]) if c and k >= s["ini"]}
            assert cst == ({5} if stereo else {5, 6})
    finally:
        dm.close()


def test_batched_setup_equals_single_calls(ctx):
    """six maps in one call == six single calls, array for array"""
    names = ["12kf", "70kf", "one", "empty", "12kf", "70kf"]
    ss = [scene(n, True, seed=SCENES[n]["seed"] + 10 * i) for i, n in enumerate(names)]
    maps, twins = [LC.build_device(ctx, s) for s in ss], [LC.build_device(ctx, s) for s in ss]
    try:
        maps[4].remove_keyframe(3); twins[4].remove_keyframe(3)
        vs = DM.loose_setup_batch(ctx, maps, [s["ini"] for s in ss], [s["n"] for s in ss], 1, True, ss[0]["P"].calib_l)
        for b, (s, t) in enumerate(zip(ss, twins)):
            got = DM.fetch_view(ctx, vs[b], True)
            _, ref = setup_one(ctx, t, s)
            assert sorted(got) == sorted(ref)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (b, k)
    finally:
        for m in maps + twins:
            m.close()


# ---- update alone ---------------------------------------------------------------------------------------------------
def upload_state(ctx, v, pose, lm):
    for ptr, a in ((v.pose, pose), (v.lm, lm)):
        a = np.ascontiguousarray(a, np.float64)
        assert ctx.lib.ov2_memcpy_h2d(ctx.h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0


@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", ["12kf", "70kf"])
def test_update_alone_equals_apply_loose_ba(ctx, name, inv_depth):
    """the same crafted "solved" state and flags through Optimizer::applyLooseBA + flush and through
    ov2_map_loose_ba_update_batch: the same survivors, states and stereo flags; poses, T_corr, propagated points and XYZ points
    and the inverse-depth points of step 2 bitwise (measured: they need no tolerance); the record's counts and lists are the
    differences of the two states"""
    s = scene(name, inv_depth)
    hm, href = LC.build_host(s), LC.build_host(s)
    hm.attach_device(ctx)
    hm.flush_device()
    dm = LC.build_device(ctx, s)
    try:
        adopt_points(dm, hm)
        start = DM.canonical_state(dm.download())
        hpb = href.setup_range_ba(s["ini"], s["n"], kf_obs_max=s["n"], min_obs=0)
        v, dpb = setup_one(ctx, dm, s)
        cs = LC.crafted(s, dpb)
        Th = hm.apply_loose_ba(s["ini"], s["n"], *LC.in_order(hpb, cs))
        assert Th is not None
        hm.flush_device()
        ref = DM.canonical_state(_Handle(ctx, hm.device_handle()).download())
        pose, lm, flags = LC.in_order(dpb, cs)
        upload_state(ctx, v[0], pose, lm)
        r = DM.loose_update_batch(ctx, [dm], v, cur_kfid=[s["cur_kfid"]], outliers=[flags])[0]
        got = DM.canonical_state(dm.download())
        kf_r, lm_r, ob_r = ref
        kf_g, lm_g, ob_g = got
        assert sorted(kf_r) == sorted(kf_g) and sorted(lm_r) == sorted(lm_g), "surviving keyframes / landmarks differ"
        assert ob_r == ob_g, "surviving observations / stereo flags differ"
        assert kf_r == kf_g, "poses differ (bitwise)"
        for l in lm_r:   # step 2's inverse-depth points came out bitwise as well: one assertion for every point
            assert lm_r[l] == lm_g[l], (l, lm_r[l], lm_g[l])
        # T_corr = opt * inverse(old(nkfid)): bitwise the host stage's, and it takes the old pose of the loop keyframe to the
        # solved one (to rounding: one more SE(3) product)
        assert np.array_equal(r["T_corr"].view(np.uint64), Th.view(np.uint64)), (r["T_corr"], Th)
        opt = pose[list(dpb["pose_kfid"]).index(s["n"])]
        assert np.allclose(LR.mat(r["T_corr"]) @ LR.mat(np.array(start[0][s["n"]])), LR.mat(opt), rtol=0, atol=1e-12)
        d1 = LR.setup(LC.snapshot(s), s["ini"], s["n"], 1, inv_depth)[1]
        _, cnt, _ = LR.update(d1, dpb, pose, lm, flags, s["n"], s["cur_kfid"], s["P"].calib_l, inv_depth)
        # the record against the two downloaded states, and against the numpy statement
        kf_s, lm_s, ob_s = start
        removed = set(lm_s) - set(lm_g)
        gone = {(int(k), int(l)) for k, l in r["removed_obs"]}
        demoted = {(int(k), int(l)) for k, l in r["stereo_off"]}
        assert r["n_removed_lm"] == len(removed) and set(r["removed_lmid"].tolist()) == removed
        assert len(gone) == r["n_removed_obs"] and len(demoted) == r["n_stereo_off"]   # each observation at most once
        assert set(ob_s) - set(ob_g) == gone | {o for o in ob_s if o[1] in removed}     # the rows of a removed landmark go with it
        assert {o for o in ob_g if ob_s[o] and not ob_g[o]} == {o for o in demoted if o[1] in lm_g}
        for k in ("n_flagged_left", "n_flagged_right", "n_removed_obs", "n_stereo_off", "n_removed_lm", "n_written", "n_propagated",
                  "n_kf_younger", "n_bad", "ran"):
            assert r[k] == cnt[k], (k, r[k], cnt[k])
        assert r["n_propagated"] > 0 and r["n_removed_lm"] > 0 and r["n_removed_obs"] > 0 and r["n_stereo_off"] > 0
        assert (r["n_pose"], r["n_lm"], r["n_res"]) == (v[0].n_pose, v[0].n_lm, v[0].n_res)
        assert r["n_free_pose"] == int(np.sum(dpb["pose_const"] == 0))
    finally:
        dm.close()


# ---- the whole statement --------------------------------------------------------------------------------------------
def assert_close_states(ref, got):
    kf_r, lm_r, ob_r = ref
    kf_g, lm_g, ob_g = got
    assert sorted(kf_r) == sorted(kf_g) and sorted(lm_r) == sorted(lm_g), "surviving keyframes / landmarks differ"
    assert ob_r == ob_g, "surviving observations / stereo flags differ"
    dp = max(float(np.max(np.abs(LR.mat(np.array(kf_r[k])) - LR.mat(np.array(kf_g[k]))))) for k in kf_r)
    dl = 0.0
    for l in lm_r:
        assert lm_r[l][1] == lm_g[l][1], l
        a, b = np.array(lm_r[l][0]), np.array(lm_g[l][0])
        dl = max(dl, float(np.max(np.abs(a - b)) / max(np.linalg.norm(a), 1e-300)))
    return dp, dl


@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", ["12kf", "70kf"])
def test_whole_statement_equals_the_host_stage(ctx, name, inv_depth):
    s = scene(name, inv_depth)
    hm = LC.build_host(s)
    hm.attach_device(ctx)
    hm.flush_device()
    dm = LC.build_device(ctx, s)
    try:
        adopt_points(dm, hm)
        st, n1, fc = hm.loose_ba(ctx, s["ini"], s["n"])
        assert st == 0 and n1 > 0
        hm.flush_device()
        ref = DM.canonical_state(_Handle(ctx, hm.device_handle()).download())
        r = dm.loose_ba_batch(inikfid=[s["ini"]], nkfid=[s["n"]], inv_depth=inv_depth, cur_kfid=[s["cur_kfid"]])[0]
        assert r["ran"] == 1 and r["n_outliers_pass1"] == n1
        assert r["n_flagged_left"] + r["n_flagged_right"] == n1
        assert r["final_cost"] == pytest.approx(fc, rel=1e-9) and 1 < r["n_log"] <= 6
        dp, dl = assert_close_states(ref, DM.canonical_state(dm.download()))
        print(f"[loose BA {name} inv={inv_depth}] host form vs mirror form: poses {dp:.2e}, points {dl:.2e} relative; n_outliers {n1}")
        assert dp <= LOOSE_POSE_TOL and dl <= LOOSE_POINT_TOL, (dp, dl)
    finally:
        dm.close()


def test_batch_independence_and_repeatability(ctx):
    """four distinct maps in one call == four single calls (tables bitwise, records and logs equal); the same batch twice
    from the same saved state is bitwise the same"""
    ss = [scene("12kf", True), scene("70kf", True), scene("12kf", True, seed=77, ini=2, n=9), scene("empty", True)]
    maps, twins = [LC.build_device(ctx, s) for s in ss], [LC.build_device(ctx, s) for s in ss]
    cams = [DM.SbaCamC.of(s["P"]) for s in ss]
    try:
        for m in maps:
            m.save_state()
        before = [m.download() for m in maps]
        args = ([s["ini"] for s in ss], [s["n"] for s in ss], cams)
        r1 = DM.loose_ba_batch(ctx, maps, *args, cur_kfid=[s["cur_kfid"] for s in ss])
        d1 = [m.download() for m in maps]
        for b, (s, t) in enumerate(zip(ss, twins)):
            r = DM.loose_ba_batch(ctx, [t], [s["ini"]], [s["n"]], [cams[b]], cur_kfid=[s["cur_kfid"]])[0]
            assert r["raw"] == r1[b]["raw"], b
            assert same_tables(d1[b], t.download()), b
        assert [r["ran"] for r in r1] == [1, 1, 1, 0] and r1[3]["termination"] == 6
        assert same_tables(before[3], d1[3])                       # the no-op map inside a batch whose other maps run
        assert not same_tables(before[0], d1[0])
        DM.restore_state_batch(ctx, maps)
        for b, m in enumerate(maps):
            assert same_tables(before[b], m.download()), b         # save_state covers everything the statement writes
        r2 = DM.loose_ba_batch(ctx, maps, *args, cur_kfid=[s["cur_kfid"] for s in ss])
        for b, m in enumerate(maps):
            assert r2[b]["raw"] == r1[b]["raw"] and same_tables(d1[b], m.download()), b
    finally:
        for m in maps + twins:
            m.close()


def build_device_reordered(ctx, s):
    """build_device with the rows of every keyframe in descending lmid, the keyframes in descending kfid"""
    P = s["P"]
    kf, lm, un, st, run = DM.observations_of(P)
    nk, nl = len(P.pose), len(P.lm)
    m = DM.DeviceMap(ctx, nk + 8, nl + 8, len(kf) + 64)
    m.prob, m.newkf = P, nk - 1
    m.set_landmarks(np.arange(nl, dtype=np.int32), DM.world_points_of(P), np.full(nl, DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D | DM.LM_OBS, np.uint8))
    cut = np.searchsorted(kf, np.arange(nk + 1))
    for k in range(nk - 1, -1, -1):
        sl = slice(cut[k], cut[k + 1])
        m.add_keyframe(k, P.pose[k], lm[sl][::-1], un[sl][::-1], run[sl][::-1], st[sl][::-1])
    if len(s["rm_kf"]):
        m.remove_obs(s["rm_kf"], s["rm_lm"])
    off = np.asarray(s["isobs_off"], np.int32)
    m.set_landmarks(off, None, np.full(len(off), DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D, np.uint8))
    return m


@pytest.mark.parametrize("inv_depth", [True, False])
def test_another_row_order_of_the_tables(ctx, inv_depth):
    """the same rows in another order: the same set-up keyed by ids, the same survivors, states within the measured
    tolerance"""
    s = scene("12kf", inv_depth)
    a, b = LC.build_device(ctx, s), build_device_reordered(ctx, s)
    try:
        assert not np.array_equal(a.download()["obs_lm"], b.download()["obs_lm"])
        _, pa = setup_one(ctx, a, s)
        _, pb = setup_one(ctx, b, s)
        assert_same_problem(pa, pb, inv_depth, exact=True)
        assert np.array_equal(pa["bad_lmid"], pb["bad_lmid"])
        ra = a.loose_ba_batch(inikfid=[s["ini"]], nkfid=[s["n"]], inv_depth=inv_depth, cur_kfid=[s["cur_kfid"]])[0]
        rb = b.loose_ba_batch(inikfid=[s["ini"]], nkfid=[s["n"]], inv_depth=inv_depth, cur_kfid=[s["cur_kfid"]])[0]
        assert all(ra[k] == rb[k] for k in DM._LOOSE_COUNTS if k != "n_log")
        dp, dl = assert_close_states(DM.canonical_state(a.download()), DM.canonical_state(b.download()))
        print(f"[loose BA row order inv={inv_depth}] poses {dp:.2e}, points {dl:.2e} relative")
        assert dp <= LOOSE_POSE_TOL and dl <= LOOSE_POINT_TOL, (dp, dl)
    finally:
        a.close(); b.close()


# ---- the chain of a loop closure on a mirror-only map -----------------------------------------------------------------
def test_chain_of_the_four_statements_on_a_mirror(ctx):
    """pose-graph update -> merge -> structure-only BA -> loose BA enqueued one behind the other == the same four calls with
    a download between each, bitwise (the host chain's row order differs by design: DESIGN.md section 8)"""
    s = synth_close.make_scene(1, "big")
    NEWKF, START = synth_close.NEWKF, synth_close.LOOSE_START
    newkf, lckf, pairs0 = synth_revisit.verify_pairs(s)["accept"]

    def mirror():
        m = host_map.LoopMap(s)
        v = m.loop_verify_candidate(ctx, newkf, lckf, pairs0, 5, nransac_iter=synth_revisit.NRANSAC_ITER, fransac_err=synth_revisit.FRANSAC_ERR)
        m.attach_device(ctx)
        return m, _Handle(ctx, m.device_handle()), v
    A, hA, v = mirror()
    B, hB, _ = mirror()
    try:
        pairs = np.array([(p, n) for p, n in v["final"] if p != n], np.int32)
        ids = np.array([k for k in sorted(s["kfids"]) if synth_close.INIKF < k <= NEWKF], np.int32)
        d0 = hA.download()
        rng = np.random.default_rng(3)
        Twc = d0["kf_pose"][ids].copy()
        Twc[:, :3] += rng.normal(0, 0.02, (len(ids), 3))
        cam = DM.SbaCamC()
        cam.calib_l[:], cam.calib_r[:], cam.T_rl[:] = list(s["K4"]), list(s["K4"]), [-0.11, 0, 0, 0, 0, 0, 1.0]
        merged = pairs[:, 1].copy()

        def chain(h, between):
            DM.pose_graph_update_batch(ctx, [h], [NEWKF], [ids], [Twc], want_header=False); between()
            DM.merge_points_batch(ctx, [h], [pairs], want_header=False); between()
            DM.structure_ba_batch(ctx, [h], [merged], [cam], want_header=False); between()
            return DM.loose_ba_batch(ctx, [h], [START], [NEWKF], [cam], cur_kfid=[-1])[0]
        ra = chain(hA, lambda: None)
        rb = chain(hB, lambda: hB.download())
        assert ra["raw"] == rb["raw"] and ra["ran"] == 1 and ra["n_res"] > 0
        da = hA.download()
        assert same_tables(da, hB.download()) and not same_tables(d0, da)
    finally:
        A.close(); B.close()


# ---- interactions and refusals --------------------------------------------------------------------------------------
def test_interactions_and_refusals(ctx):
    from ov2slam_amd import frontend
    s = scene("12kf", True)
    dm, other = LC.build_device(ctx, s), LC.build_device(ctx, s)
    ctx2 = frontend.Context(0)
    alien = LC.build_device(ctx2, s)
    try:
        L = ctx.lib
        K4 = np.ascontiguousarray(s["P"].calib_l, np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        i32 = lambda *a: np.array(a, np.int32)

        def setup(hs, lo, hi, B=None, views=True):
            n = len(hs)
            return L.ov2_map_loose_ba_setup_batch(ctx.h, n if B is None else B, (C.c_void_p * max(n, 1))(*hs), None if lo is None else vp(i32(*lo)),
                                                  None if hi is None else vp(i32(*hi)), 1, 1, vp(np.tile(K4, (max(n, 1), 1))),
                                                  (DM.SetupC * max(n, 1))() if views else None)

        def loose_update(h):
            return L.ov2_map_loose_ba_update_batch(ctx.h, 1, (C.c_void_p * 1)(h), (C.c_void_p * 1)(None), None, None, None)

        def local_update(h):
            return L.ov2_map_local_ba_update_batch(ctx.h, 1, (C.c_void_p * 1)(h), (C.c_void_p * 1)(None), None, None)

        def launches(call):
            """(status, kernels the call enqueued), from the context's kernel timer"""
            ctx.synchronize()
            ctx.kernel_timing(True); ctx.kernel_times()
            st = call()
            n = sum(v[1] for v in ctx.kernel_times().values())
            ctx.kernel_timing(False)
            return st, n
        refused = lambda call: launches(call) == (INVALID, 0)
        before, before_other = dm.download(), other.download()
        assert refused(lambda: loose_update(dm.h))                              # no set-up at all
        assert refused(lambda: setup([dm.h], [3], [40]))                        # nkfid out of range
        assert refused(lambda: setup([dm.h], [-1], [8]))                        # inikfid < 0
        assert refused(lambda: setup([other.h, dm.h, other.h], [3, 3, 3], [8, 8, 8]))   # a map listed twice
        assert refused(lambda: setup([dm.h, alien.h], [3, 3], [8, 8]))          # a map of another context
        assert refused(lambda: setup([dm.h], [3], [8], B=-1))
        assert refused(lambda: setup([dm.h], None, [8])) and refused(lambda: setup([dm.h], [3], None))
        assert refused(lambda: setup([dm.h], [3], [8], views=False))
        other.remove_keyframe(8)
        before_other = other.download()
        assert refused(lambda: setup([other.h], [3], [8]))                      # nkfid dead
        assert same_tables(before, dm.download()) and same_tables(before_other, other.download())
        assert refused(lambda: loose_update(dm.h))                              # ... and none of them left a set-up behind
        assert launches(lambda: setup([], [], [], B=0)) == (0, 0)
        # a local update after a loose set-up, and the reverse
        st, n = launches(lambda: setup([dm.h], [3], [8]))
        assert st == 0 and n == 15                                              # the timer does see the chain of an accepted call
        after_setup = dm.download()
        assert refused(lambda: local_update(dm.h)) and same_tables(after_setup, dm.download())
        assert launches(lambda: loose_update(dm.h)) == (0, 7)                   # both outputs NULL: no gather launch
        assert refused(lambda: loose_update(dm.h))                              # a second loose update of one set-up
        DM.setup_batch(ctx, [dm], inv_depth=True, calib_l=K4)
        after_setup = dm.download()
        assert refused(lambda: loose_update(dm.h)) and same_tables(after_setup, dm.download())
        assert local_update(dm.h) == 0
        # the asynchronous form (both outputs NULL) leaves what the synchronous one leaves
        a, b = LC.build_device(ctx, s), LC.build_device(ctx, s)
        try:
            va, pa = setup_one(ctx, a, s)
            vb, _ = setup_one(ctx, b, s)
            cs = LC.crafted(s, pa)
            pose, lm, flags = LC.in_order(pa, cs)
            upload_state(ctx, va[0], pose, lm); upload_state(ctx, vb[0], pose, lm)
            assert DM.loose_update_batch(ctx, [a], va, cur_kfid=[8], outliers=[flags], want=False) is None
            assert DM.loose_update_batch(ctx, [b], vb, cur_kfid=[8], outliers=[flags])[0]["ran"] == 1
            assert same_tables(a.download(), b.download())
        finally:
            a.close(); b.close()
    finally:
        dm.close(); other.close(); alien.close(); ctx2.close()
