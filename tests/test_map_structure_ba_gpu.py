"""Optimizer::structureOnlyBA on the map mirrors (ov2_map_structure_ba_batch / _dev, reference src/optimizer.cpp:2594-2781):
parity per case against the oracle's solve of the flat problem the checker builds from the downloaded tables
(tests/structure_ba_ref.py, cases and their tameness: tests/structure_ba_cases.py, tests/test_structure_ba_ref_cpu.py), against
the C++ host stage, batches in both orders and alone, the row order of the table, lists with entries that do not enter, the
device-side forms and the chain behind a merge, the interactions with the set-up / update and saved states, refusals, and
the asynchronous form.
Tolerances, those of tests/test_host_adapter.py::test_structure_only_ba: costs to 1e-9 relative, points to
1e-9 * max(1, |x|_inf); flags, termination and counts exact; everything the stage promises to repeat is compared bitwise."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import ba_types as T, device_map as DM, host_map
import structure_ba_cases as SC
import structure_ba_ref as SR
from test_structure_ba_ref_cpu import POINT_TOL, point_error, reference

pytestmark = pytest.mark.gpu
INVALID = -1   # OV2_ERR_INVALID (include/ov2slam_hip.h)
TABLES = ("kf_pose", "kf_state", "lm_xyz", "lm_state", "obs_kf", "obs_lm", "obs_flag", "obs_uv", "obs_ruv")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def same_tables(a, b, but_points_of=()):
    """byte for byte, but for the points of the landmarks named; slots that hold nothing were never written"""
    if not all(np.array_equal(a[k], b[k]) for k in TABLES if k not in ("kf_pose", "lm_xyz")):
        return False
    kf, lm = a["kf_state"] != 0, (a["lm_state"] & DM.LM_ALIVE) != 0
    lm[np.asarray(but_points_of, np.int64)] = False
    return np.array_equal(a["kf_pose"][kf].view(np.uint64), b["kf_pose"][kf].view(np.uint64)) and \
        np.array_equal(a["lm_xyz"][lm].view(np.uint64), b["lm_xyz"][lm].view(np.uint64))


def cam_of(name):
    return DM.SbaCamC.of(SC.problem_of(name)[0])


def options(ctx, name):
    return DM.structure_ba_options(ctx, SC.CASES[name]["max_iters"])


def run_case(ctx, dm, name, ids=None, **kw):
    ids = SC.problem_of(name)[2] if ids is None else ids
    return DM.structure_ba_batch(ctx, [dm], [ids], [cam_of(name)], options(ctx, name), **kw)


def flags(h):
    return [(int(i["valid"]), int(i["ok"])) for i in h["log"]]


def assert_matches_oracle(h, points, ref):
    """costs, flags, termination, counts and points of one map against the oracle's solve"""
    R = ref["result"]
    print("header", {k: h[k] for k in h if k not in ("log", "raw")}, "oracle", ref["counts"], R.c.initial_cost, R.c.final_cost,
          "points", point_error(points, ref["points"]))
    assert {k: h[k] for k in ("n_listed", "n_lm", "n_skipped", "n_res")} == ref["counts"]
    assert h["termination"] == R.c.termination and h["n_log"] == R.c.n_log and flags(h) == ref["flags"]
    assert h["initial_cost"] == pytest.approx(R.c.initial_cost, rel=1e-9) and h["final_cost"] == pytest.approx(R.c.final_cost, rel=1e-9)
    assert point_error(points, ref["points"]) <= POINT_TOL


@pytest.mark.parametrize("name", SC.SHAPES + SC.BRANCHES)
def test_parity_with_the_oracle(ctx, name):
    ref = reference(name)
    dm = SC.mirror_of(ctx, name)
    try:
        d0 = dm.download()
        model, scale = SC.tables_of(name)
        assert same_tables(d0, model) and np.array_equal(dm.row_scale, scale)   # the checker sees the mirror's tables
        h = run_case(ctx, dm, name)[0]
        d1 = dm.download()
        assert_matches_oracle(h, d1["lm_xyz"][ref["ids"]], ref)
        assert same_tables(d0, d1, but_points_of=ref["ids"])
        if SC.CASES[name]["max_iters"] == 0:
            assert same_tables(d0, d1)
        else:
            assert not same_tables(d0, d1)
        used = DM.SbaC.log.offset + h["n_log"] * C.sizeof(T.BaIterC)   # zeros behind n_log
        assert h["raw"][used:] == bytes(C.sizeof(DM.SbaC) - used)
    finally:
        dm.close()


def test_equals_the_host_stage(ctx, oracle):
    """HostMap.structure_only_ba -- the general local-BA solver on the flat problem of the C++ host mirror -- on the first
    shape as the host test runs it (no noise, every level 0): same cost, same points, both within the tolerance of the oracle"""
    P = SC.problem_of("w10x400")[0]
    ids = SC.problem_of("w10x400")[2]
    hm = host_map.HostMap(P)
    dm = DM.DeviceMap.from_problem(ctx, P)
    try:
        st, cost, its = hm.structure_only_ba(ctx, ids)
        assert st == 0
        Q, R, counts, entered = SR.solve(oracle, dm.download(), dm.row_scale, ids, SC.cam_of("w10x400"))
        h = dm.structure_ba_batch(lmids=[ids])[0]
        pts = dm.download()["lm_xyz"][ids]
        ref = dict(result=R, counts=counts, points=Q.lm, flags=[(int(i["valid"]), int(i["ok"])) for i in R.log])
        assert_matches_oracle(h, pts, ref)
        host_pts = np.array([hm.landmark(int(l))[0] for l in ids])
        print("host stage: cost", cost, "iterations", its, "points against the mirror", point_error(pts, host_pts))
        assert h["final_cost"] == pytest.approx(cost, rel=1e-9) and its == h["n_log"] - 1
        assert point_error(pts, host_pts) <= POINT_TOL and point_error(host_pts, Q.lm) <= POINT_TOL
    finally:
        dm.close()
        del hm


def test_batch_independence_and_repeatability(ctx):
    names = ["w10x400", "w3x8", "w10x2600"]
    maps = [SC.mirror_of(ctx, n) for n in names]
    lists = [np.zeros(0, np.int32), SC.problem_of("w3x8")[2], SC.problem_of("w10x2600")[2]]
    cams = [cam_of(n) for n in names]
    try:
        for m in maps:
            m.save_state()
        before = [m.download() for m in maps]

        def run(order):
            DM.restore_state_batch(ctx, maps)
            hs = DM.structure_ba_batch(ctx, [maps[b] for b in order], [lists[b] for b in order], [cams[b] for b in order])
            return {b: (maps[b].download(), hs[i]) for i, b in enumerate(order)}
        fwd, rev, again = run([0, 1, 2]), run([2, 1, 0]), run([0, 1, 2])
        assert fwd[0][1]["termination"] == 6 and fwd[0][1]["n_listed"] == 0 and fwd[0][1]["raw"] == bytes(DM.SbaC(termination=6))
        assert same_tables(before[0], fwd[0][0])
        assert fwd[1][1]["n_lm"] == 8 and fwd[2][1]["n_lm"] == 1300 and fwd[2][1]["n_log"] > 2
        for b in range(3):
            alone = run([b])[b]
            for other in (rev[b], again[b], alone):
                assert same_tables(fwd[b][0], other[0]) and fwd[b][1]["raw"] == other[1]["raw"], b
        for b in (1, 2):
            assert_matches_oracle(fwd[b][1], fwd[b][0]["lm_xyz"][lists[b]], reference(names[b]))
    finally:
        for m in maps:
            m.close()


def test_row_order_of_the_table(ctx):
    """part of keyframe 2's rows appended after all keyframes stand (as merges and late matches append them): the rows of a
    point are no longer in keyframe order in the table, the result is bitwise the same"""
    name = "w10x400"
    P, scale, ids, xyz, _, _ = SC.problem_of(name)
    a = SC.mirror_of(ctx, name)
    kf, lm, un, st, run = DM.observations_of(P)
    nk, nl = len(P.pose), len(P.lm)
    b = DM.DeviceMap(ctx, nk + 8, nl + 8, len(kf) + 64)
    try:
        b.set_landmarks(np.arange(nl, dtype=np.int32), DM.world_points_of(P), SC.tables_of(name, noisy=False)[0]["lm_state"][:nl])
        late = (kf == 2) & (np.arange(len(kf)) % 2 == 1)
        for k in range(nk):
            s = (kf == k) & ~late
            b.add_keyframe(k, P.pose[k], lm[s], un[s], run[s], st[s], scale[s])
        b.add_keyframe(2, P.pose[2], lm[late], un[late], run[late], st[late], scale[late])
        b.set_landmarks(ids, xyz, SC.tables_of(name)[0]["lm_state"][ids])
        db = b.download()
        assert not np.array_equal(db["obs_kf"], kf) and late.sum() > 50
        assert np.isin(lm[late], ids).sum() > 20
        ha, hb = run_case(ctx, a, name)[0], run_case(ctx, b, name)[0]
        da, db = a.download(), b.download()
        assert ha["raw"] == hb["raw"] and ha["n_lm"] == len(ids)
        assert np.array_equal(da["lm_xyz"][:nl].view(np.uint64), db["lm_xyz"][:nl].view(np.uint64))
    finally:
        a.close(); b.close()


def test_lists_with_entries_that_do_not_enter(ctx, oracle):
    name = "w10x400"
    ids = SC.problem_of(name)[2]
    dm = SC.mirror_of(ctx, name)
    try:
        dead, flat, bare = ids[3:6], ids[10:13], ids[20:22]
        dm.remove_landmarks(dead)
        dm.set_landmarks(flat, None, np.full(len(flat), DM.LM_ALIVE, np.uint8))
        kf, lm = DM.observations_of(SC.problem_of(name)[0])[:2]
        dm.remove_obs(kf[np.isin(lm, bare)], lm[np.isin(lm, bare)])
        dm.save_state()
        d0 = dm.download()
        nl = len(d0["lm_state"])
        junk = np.concatenate([[-3, nl, 10 ** 6], ids[:30], [ids[0], ids[7], ids[7]], ids[30:], [ids[40], nl - 1]]).astype(np.int32)
        entered, counts = SR.select(d0, junk)
        assert counts["n_skipped"] == 3 + 8 + 3 + 2 and ids[0] in entered and not set(entered) & set(np.concatenate([dead, flat, bare]).tolist())
        h = run_case(ctx, dm, name, junk)[0]
        d1 = dm.download()
        assert {k: h[k] for k in ("n_listed", "n_lm", "n_skipped")} == counts
        assert same_tables(d0, d1, but_points_of=entered) and not same_tables(d0, d1)
        DM.restore_state_batch(ctx, [dm])
        h2 = run_case(ctx, dm, name, np.array(entered, np.int32))[0]
        assert h2["n_skipped"] == 0 and h2["n_lm"] == h["n_lm"] and h2["n_res"] == h["n_res"]
        assert same_tables(d1, dm.download()) and h2["log"] == h["log"] and h2["final_cost"] == h["final_cost"]
        # against the oracle on the tables as they stood
        P, R, c2, _ = SR.solve(oracle, d0, dm.row_scale, junk, SC.cam_of(name))
        assert_matches_oracle(h, d1["lm_xyz"][entered], dict(result=R, counts=c2, points=P.lm, flags=[(int(i["valid"]), int(i["ok"])) for i in R.log]))
        # a list of which nothing enters: counted, skipped, nothing touched
        DM.restore_state_batch(ctx, [dm])
        h3 = run_case(ctx, dm, name, np.concatenate([dead, flat, bare, [-1]]).astype(np.int32))[0]
        assert (h3["n_listed"], h3["n_lm"], h3["n_skipped"], h3["n_res"], h3["termination"], h3["n_log"]) == (9, 0, 9, 0, 6, 0)
        assert same_tables(d0, dm.download())
    finally:
        dm.close()


def test_device_form_count_and_status(ctx):
    name = "w10x400"
    ids = SC.problem_of(name)[2]
    dm, twin = SC.mirror_of(ctx, name), SC.mirror_of(ctx, name)
    try:
        seg = np.concatenate([ids[:90], [ids[5], -1], ids[90:]]).astype(np.int32)
        n = 120
        status = (np.arange(len(seg)) % 7 == 3).astype(np.uint8) * DM.MERGE_SKIP_NEW_DEAD
        status[len(seg) - 1] = DM.MERGE_DONE
        dev = DM.DevIds([0, len(seg)], ctx.to_device(seg), ctx.to_device(np.array([n], np.int32)))
        h = DM.structure_ba_batch(ctx, [dm], dev, [cam_of(name)], dev=True, d_status=ctx.to_device(status))[0]
        same = seg[:n][status[:n] == DM.MERGE_DONE]
        h2 = DM.structure_ba_batch(ctx, [twin], [same], [cam_of(name)])[0]
        print({k: h[k] for k in h if k not in ("log", "raw")})
        assert h["raw"] == h2["raw"] and h["n_listed"] == len(same) and h["n_skipped"] == 2 and h["n_lm"] > 90
        assert same_tables(dm.download(), twin.download())
        # a count beyond the segment is clamped to it, a negative one to nothing
        dev = DM.DevIds([0, len(seg)], ctx.to_device(seg), ctx.to_device(np.array([10 ** 6], np.int32)))
        assert DM.structure_ba_batch(ctx, [dm], dev, [cam_of(name)], dev=True)[0]["n_listed"] == len(seg)
        dev = DM.DevIds([0, len(seg)], ctx.to_device(seg), ctx.to_device(np.array([-5], np.int32)))
        before = dm.download()
        h = DM.structure_ba_batch(ctx, [dm], dev, [cam_of(name)], dev=True)[0]
        assert (h["n_listed"], h["termination"]) == (0, 6) and same_tables(before, dm.download())
    finally:
        dm.close(); twin.close()


def test_chain_behind_a_merge_on_the_device(ctx):
    """merge_points_batch_dev -> structure_ba_batch_dev on its new ids, its device-side count and its status bytes, with no host
    read in between == the two host-form calls one after the other"""
    name = "w10x400"
    ids = SC.problem_of(name)[2]
    maps, twins = [SC.mirror_of(ctx, name), SC.mirror_of(ctx, "w3x8")], [SC.mirror_of(ctx, name), SC.mirror_of(ctx, "w3x8")]
    cams = [cam_of(name), cam_of("w3x8")]
    try:
        # (prev, new): odd ids merge into their even neighbours; a pair on itself, a dead `prev` and a pair beyond the count
        p0 = np.array([(ids[i] + 1, ids[i]) for i in range(0, 60, 2)] + [(ids[70], ids[70]), (ids[0] + 1, ids[72]), (ids[81] + 1 - 1, ids[80])], np.int32)
        p1 = np.array([(1, 0), (3, 2), (5, 4)], np.int32)
        cut = [len(p0) - 1, 2]
        off = np.array([0, len(p0), len(p0) + len(p1)], np.int32)
        flat = np.concatenate([p0, p1])
        d_prev, d_new, d_n = ctx.to_device(flat[:, 0].copy()), ctx.to_device(flat[:, 1].copy()), ctx.to_device(np.array(cut, np.int32))
        d_st = ctx.to_device(np.full(len(flat), DM.MERGE_NOT_RUN, np.uint8))
        hs = (C.c_void_p * 2)(*[m.h for m in maps])
        assert ctx.lib.ov2_map_merge_points_batch_dev(ctx.h, 2, hs, off.ctypes.data_as(C.c_void_p), d_prev.ptr, d_new.ptr, None, d_n.ptr,
                                                      None, d_st.ptr) == 0
        assert DM.structure_ba_batch(ctx, maps, DM.DevIds(off, d_new, d_n), cams, dev=True, d_status=d_st, want_header=False) is None
        hdr, st = DM.merge_points_batch(ctx, twins, [p0[:cut[0]], p1[:cut[1]]])
        assert hdr[0]["n_merged"] == 30 and hdr[0]["n_skipped"] == 2 and hdr[1]["n_merged"] == 2
        lists = [p0[:cut[0], 1][st[0] == DM.MERGE_DONE], p1[:cut[1], 1][st[1] == DM.MERGE_DONE]]
        h = DM.structure_ba_batch(ctx, twins, lists, cams)
        assert h[0]["n_lm"] == 30 and h[1]["n_lm"] == 2 and h[0]["n_log"] > 2
        for a, b in zip(maps, twins):
            assert same_tables(a.download(), b.download())
    finally:
        for m in maps + twins:
            m.close()


def test_interactions_with_the_set_up_and_saved_states(ctx):
    name = "w10x400"
    ids = SC.problem_of(name)[2]
    K4 = SC.problem_of(name)[0].calib_l
    dm = SC.mirror_of(ctx, name)
    try:
        hs = (C.c_void_p * 1)(dm.h)
        update = lambda: ctx.lib.ov2_map_local_ba_update_batch(ctx.h, 1, hs, (C.c_void_p * 1)(None), None, None)   # no outlier flags
        DM.setup_batch(ctx, [dm], inv_depth=False, calib_l=K4)
        before = dm.download()
        h = run_case(ctx, dm, name, ids[:0])[0]
        assert h["termination"] == 6 and same_tables(before, dm.download())
        assert update() == 0                                                          # an empty segment leaves the set-up alone
        DM.setup_batch(ctx, [dm], inv_depth=False, calib_l=K4)
        run_case(ctx, dm, name)
        assert update() == INVALID
        # a saved state covers the points
        twin = SC.mirror_of(ctx, name)
        try:
            twin.save_state()
            d0 = twin.download()
            run_case(ctx, twin, name)
            assert not same_tables(d0, twin.download())
            DM.restore_state_batch(ctx, [twin])
            assert same_tables(d0, twin.download())
        finally:
            twin.close()
    finally:
        dm.close()


def test_refusals_leave_the_tables_alone(ctx):
    from ov2slam_amd import frontend
    name = "w3x8"
    ids = SC.problem_of(name)[2]
    dm, other = SC.mirror_of(ctx, name), SC.mirror_of(ctx, name)
    ctx2 = frontend.Context(0)
    alien = SC.mirror_of(ctx2, name)
    try:
        L = ctx.lib
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        n = len(ids)
        lst = np.concatenate([ids, ids]).astype(np.int32)

        def call(hs, off, lmid=lst, cam=True, max_iters=10, opt=True):
            off = np.array(off, np.int32)
            cams = (DM.SbaCamC * len(hs))(*[cam_of(name)] * len(hs))
            o = DM.structure_ba_options(ctx, max_iters)
            return L.ov2_map_structure_ba_batch(ctx.h, len(hs), (C.c_void_p * len(hs))(*hs), vp(off), None if lmid is None else vp(lmid),
                                                cams if cam else None, C.byref(o) if opt else None, (DM.SbaC * len(hs))())
        before, before_other = dm.download(), other.download()
        assert call([other.h, dm.h, other.h], [0, 2, 4, 6]) == INVALID       # a map listed twice
        assert call([dm.h, other.h], [0, 6, 3]) == INVALID                    # lm_off decreases
        assert call([dm.h], [1, n]) == INVALID                                # ... or does not start at 0
        assert call([dm.h, alien.h], [0, n, 2 * n]) == INVALID                # a map of another context
        assert L.ov2_map_structure_ba_batch(ctx.h, -1, None, None, None, None, None, None) == INVALID
        assert call([dm.h], [0, n], lmid=None) == INVALID                     # null arrays that a non-empty call needs
        assert call([dm.h], [0, n], cam=False) == INVALID
        assert call([dm.h], [0, n], opt=False) == INVALID
        assert call([dm.h], [0, n], max_iters=-1) == INVALID                  # max_iters outside [0, OV2_BA_MAX_LOG - 1]
        assert call([dm.h], [0, n], max_iters=T.MAX_LOG) == INVALID
        assert L.ov2_map_structure_ba_batch_dev(ctx.h, 1, (C.c_void_p * 1)(dm.h), vp(np.array([0, n], np.int32)), None, None, None, None, None,
                                                None) == INVALID
        assert same_tables(before, dm.download()) and same_tables(before_other, other.download())
        assert L.ov2_map_structure_ba_batch(ctx.h, 0, None, None, None, None, None, None) == 0
        assert call([dm.h], [0, 0]) == 0 and call([dm.h], [0, 0], lmid=None, cam=False, opt=False) == 0   # empty lists
        assert same_tables(before, dm.download())
        assert call([dm.h], [0, n], max_iters=T.MAX_LOG - 1) == 0 and not same_tables(before, dm.download())   # and the map still works
    finally:
        dm.close(); other.close(); alien.close(); ctx2.close()


def test_asynchronous_form(ctx):
    name = "w10x2600"
    dm, twin = SC.mirror_of(ctx, name), SC.mirror_of(ctx, name)
    try:
        assert run_case(ctx, dm, name, want_header=False) is None   # out = NULL: nothing is read back, no synchronisation
        d = dm.download()                                           # the next download sees the result
        h = run_case(ctx, twin, name)[0]
        assert same_tables(d, twin.download()) and h["n_lm"] == 1300
        assert_matches_oracle(h, d["lm_xyz"][reference(name)["ids"]], reference(name))
    finally:
        dm.close(); twin.close()
