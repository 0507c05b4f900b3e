"""MapManager::mergeMapPoints on the map mirrors (ov2_map_merge_points_batch / _dev, reference src/map_manager.cpp:801-882):
the device form against the checker (tests/merge_ref.py) on the downloaded tables and against the C++ host stage feeding an
attached mirror, batches in both orders and alone, the device-side pair count, the sequential order of the pairs, the
interactions with the local-BA set-up / update, the squeeze and saved states, refusals, and the asynchronous form.  Only
index work is involved: every comparison is exact.
Maps: synth_filter.make_map (21, 60) -- 360 rows, one workgroup of rows -- and (40, 1200) -- 6082 rows, 24 workgroups of rows
and more landmarks than one 1024-wide scan block.  Lists: tests/test_merge_ref_cpu.py (hand-built + 40 / 300 random pairs)."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, host_map, synth_filter
import merge_ref as R
from test_merge_ref_cpu import MAPS, OTHER_SEED, the_map, full_list, random_pairs, host_merge, without_same

pytestmark = pytest.mark.gpu
INVALID = -1   # OV2_ERR_INVALID (include/ov2slam_hip.h)
TABLES = ("kf_pose", "kf_state", "lm_xyz", "lm_state", "obs_kf", "obs_lm", "obs_flag", "obs_uv", "obs_ruv")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


class _Borrowed:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h, newkf=-1):
        self.ctx, self.L, self.h, self.newkf = ctx, ctx.lib, h, newkf
        self._p = DM.DeviceMap._p
        self.download = lambda: DM.DeviceMap.download(self)


def fresh(ctx, key):
    return DM.DeviceMap.from_filter_map(ctx, the_map(*key)[0])


def same_tables(a, b):
    """byte for byte; the pose of a keyframe slot and the point of a landmark slot that hold nothing were never written"""
    if not all(np.array_equal(a[k], b[k]) for k in TABLES if k not in ("kf_pose", "lm_xyz")):
        return False
    kf, lm = a["kf_state"] != 0, (a["lm_state"] & DM.LM_ALIVE) != 0
    return np.array_equal(a["kf_pose"][kf].view(np.uint64), b["kf_pose"][kf].view(np.uint64)) and \
        np.array_equal(a["lm_xyz"][lm].view(np.uint64), b["lm_xyz"][lm].view(np.uint64))


def assert_equals_checker(dm, d0, pairs, cur, hdr, st):
    M = R.build(d0)
    rh, rs, _ = R.merge_list(M, pairs, cur)
    d1 = dm.download()
    print("header", hdr, "checker", rh)
    assert hdr == rh
    assert np.array_equal(st, rs)
    assert DM.canonical_state(d1) == R.canonical(M)
    assert R.row_dict_of_tables(d1) == R.row_dict(M)
    assert np.array_equal(d1["obs_lm"], M["tables"]["obs_lm"]) and np.array_equal(d1["lm_state"], M["tables"]["lm_state"])
    return d1


@pytest.mark.parametrize("key", MAPS)
@pytest.mark.parametrize("dev", [False, True])
def test_device_form_equals_checker(ctx, key, dev):
    pairs, cur, _ = full_list(*key)
    dm = fresh(ctx, key)
    try:
        d0 = dm.download()
        hdr, st = DM.merge_points_batch(ctx, [dm], [pairs], [cur], dev=dev)
        assert hdr[0]["n_rows_moved"] > 0 and hdr[0]["n_rows_conflict"] > 0
        assert_equals_checker(dm, d0, pairs, cur, hdr[0], st[0])
    finally:
        dm.close()


@pytest.mark.parametrize("key", MAPS)
def test_device_form_equals_host_stage(ctx, key):
    """two host maps with attached mirrors: one applies the list with MapManager::mergeMapPoints and flushes (a dead and an
    appended row per moved observation), the other's mirror takes the device call (rows relabelled in place)"""
    m = the_map(*key)[0]
    pairs, _, _ = full_list(*key)
    a, b = host_map.FilterMap(m), host_map.FilterMap(m)
    try:
        a.attach_device(ctx); b.attach_device(ctx)
        for p, n in without_same(pairs, pairs[:, 0])[0].tolist():
            host_merge(a, p, n)
        a.flush_device()
        mb = _Borrowed(ctx, b.device_handle())
        rows0 = len(mb.download()["obs_kf"])
        hdr, _ = DM.merge_points_batch(ctx, [mb], [pairs])
        da, db = _Borrowed(ctx, a.device_handle()).download(), mb.download()
        assert DM.canonical_state(da) == DM.canonical_state(db)
        assert R.row_dict_of_tables(da) == R.row_dict_of_tables(db)
        assert hdr[0]["n_rows_moved"] > 0 and len(db["obs_kf"]) == rows0 < len(da["obs_kf"])   # in place here, appended there
    finally:
        del a, b


def test_batch_independence_and_device_side_count(ctx):
    small, large = MAPS
    keys = [small, large, OTHER_SEED]
    lists = [(np.zeros((0, 2), np.int32), np.zeros(0, np.uint8)), full_list(*large)[:2], random_pairs(OTHER_SEED[1], 40, seed=9)]
    ps, cs = [l[0] for l in lists], [l[1] for l in lists]

    def run(order):
        maps = [fresh(ctx, keys[b]) for b in order]
        try:
            hdr, st = DM.merge_points_batch(ctx, maps, [ps[b] for b in order], [cs[b] for b in order])
            return {b: (maps[i].download(), hdr[i], st[i]) for i, b in enumerate(order)}
        finally:
            for m in maps:
                m.close()
    fwd, rev = run([0, 1, 2]), run([2, 1, 0])
    assert fwd[0][1] == dict(n_pairs=0, n_merged=0, n_skipped=0, n_rows_moved=0, n_rows_conflict=0) and len(fwd[0][2]) == 0
    assert fwd[1][1]["n_rows_moved"] > 0 and fwd[2][1]["n_rows_moved"] > 0
    for b in range(3):
        alone = run([b])[b]
        for other in (rev[b], alone):
            assert same_tables(fwd[b][0], other[0]) and fwd[b][1] == other[1] and np.array_equal(fwd[b][2], other[2]), b
    # the _dev form with fewer pairs than the segments hold == the host form on the truncated lists
    cut = [0, 77, 13]
    off = np.concatenate([[0], np.cumsum([len(p) for p in ps])]).astype(np.int32)
    maps, twins = [fresh(ctx, k) for k in keys], [fresh(ctx, k) for k in keys]
    try:
        flat = np.concatenate(ps)
        dp = DM.DevPairs(off, ctx.to_device(flat[:, 0].copy()), ctx.to_device(flat[:, 1].copy()), ctx.to_device(np.array(cut, np.int32)),
                         ctx.to_device(np.concatenate(cs)))
        hdr, st = DM.merge_points_batch(ctx, maps, dp, dev=True)
        hdr2, st2 = DM.merge_points_batch(ctx, twins, [p[:n] for p, n in zip(ps, cut)], [c[:n] for c, n in zip(cs, cut)])
        for b in range(3):
            assert hdr[b] == hdr2[b] and hdr[b]["n_pairs"] == cut[b]
            assert np.array_equal(st[b][:cut[b]], st2[b]) and np.all(st[b][cut[b]:] == DM.MERGE_NOT_RUN)
            assert same_tables(maps[b].download(), twins[b].download())
    finally:
        for m in maps + twins:
            m.close()


@pytest.mark.parametrize("key", MAPS)
@pytest.mark.parametrize("case", ["chain", "shared"])
def test_pairs_apply_in_list_order(ctx, key, case):
    """(a -> b), (b -> c) and (a -> n), (b -> n) with a keyframe that sees a and b: the device result is the checker's pair by
    pair, and the checker with the two pairs swapped gives other tables -- so the comparison can tell the orders apart"""
    pairs, _, names = full_list(*key)
    two = pairs[list(names[case])]
    dm = fresh(ctx, key)
    try:
        d0 = dm.download()
        hdr, st = DM.merge_points_batch(ctx, [dm], [two])
        d1 = assert_equals_checker(dm, d0, two, None, hdr[0], st[0])
        Ms = R.build(d0)
        R.merge_list(Ms, two[::-1])
        assert R.row_dict_of_tables(d1) != R.row_dict(Ms)
    finally:
        dm.close()


def _setup_problem(ctx, dm):
    v = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)[0]
    f = DM.fetch_view(ctx, v, True)
    assert not f["aborted"]
    keys = sorted(zip(f["res_kfid"].tolist(), f["res_lmid"].tolist(), f["res_type"].tolist(), f["res_uv"][:, 0].tolist(),
                      f["res_uv"][:, 1].tolist()))
    return (v.n_pose, v.n_lm, v.n_res), keys


def test_update_refused_after_a_merge_but_not_after_an_empty_one(ctx):
    key = MAPS[0]
    pairs, cur, _ = full_list(*key)
    dm = fresh(ctx, key)
    try:
        hs = (C.c_void_p * 1)(dm.h)
        update = lambda v: ctx.lib.ov2_map_local_ba_update_batch(ctx.h, 1, hs, (C.c_void_p * 1)(None), None, None)   # no outlier flags
        views = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)
        before = dm.download()
        hdr, st = DM.merge_points_batch(ctx, [dm], [pairs[:0]])
        assert hdr[0]["n_pairs"] == 0 and same_tables(before, dm.download())
        assert update(views[0]) == 0
        views = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)
        DM.merge_points_batch(ctx, [dm], [pairs], [cur])
        assert update(views[0]) == INVALID
    finally:
        dm.close()


def test_compact_and_setup_after_a_merge(ctx):
    """the squeeze drops the conflict rows like any dead row, and the local-BA set-up on the merged mirror gives the problem
    that a mirror built fresh from the merged host map gives"""
    key = MAPS[1]
    m = the_map(*key)[0]
    pairs, _, _ = full_list(*key)
    a, b = host_map.FilterMap(m), host_map.FilterMap(m)
    try:
        for p, n in without_same(pairs, pairs[:, 0])[0].tolist():
            host_merge(a, p, n)
        a.attach_device(ctx); b.attach_device(ctx)
        ma, mb = _Borrowed(ctx, a.device_handle(), m["newkf"]), _Borrowed(ctx, b.device_handle(), m["newkf"])
        hdr, _ = DM.merge_points_batch(ctx, [mb], [pairs])
        assert hdr[0]["n_rows_conflict"] > 0
        state = DM.canonical_state(mb.download())
        assert state == DM.canonical_state(ma.download())
        pa, pb = _setup_problem(ctx, ma), _setup_problem(ctx, mb)
        print("set-up (n_pose, n_lm, n_res):", pa[0], pb[0])
        assert pa[0] == pb[0] and pa[1] == pb[1] and pa[0][2] > 100
        state = DM.canonical_state(mb.download())   # (the set-up clears is3d_ of the bad landmarks in its window)
        r0, r1 = C.c_int(), C.c_int()
        assert ctx.lib.ov2_map_compact(mb.h, C.byref(r0), C.byref(r1)) == 0
        d = mb.download()
        assert DM.canonical_state(d) == state and r1.value == len(d["obs_kf"]) == len(state[2]) < r0.value
    finally:
        del a, b


def test_refusals_leave_the_tables_alone(ctx):
    key = MAPS[0]
    pairs, _, _ = full_list(*key)
    dm, other = fresh(ctx, key), fresh(ctx, key)
    try:
        L = ctx.lib
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        prev, new = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        n = len(pairs)

        def call(hs, off):
            off = np.array(off, np.int32)
            return L.ov2_map_merge_points_batch(ctx.h, len(hs), (C.c_void_p * len(hs))(*hs), vp(off), vp(prev), vp(new), None,
                                                (DM.MergeC * len(hs))(), None)
        before, before_other = dm.download(), other.download()
        assert call([other.h, dm.h, other.h], [0, 5, 10, 15]) == INVALID          # a map listed twice
        assert call([dm.h, other.h], [0, 10, 5]) == INVALID                        # pair_off decreases
        assert call([dm.h], [1, n]) == INVALID                                     # ... or does not start at 0
        assert L.ov2_map_merge_points_batch(ctx.h, -1, None, None, None, None, None, None, None) == INVALID
        assert L.ov2_map_merge_points_batch(ctx.h, 1, (C.c_void_p * 1)(dm.h), vp(np.array([0, n], np.int32)), None, vp(new), None,
                                            None, None) == INVALID                # a null list that a non-empty call needs
        other.save_state()
        assert call([dm.h, other.h], [0, 5, 10]) == INVALID                        # a map with a saved state
        assert call([other.h], [0, 0]) == INVALID                                  # ... even with nothing to do
        assert same_tables(before, dm.download()) and same_tables(before_other, other.download())
        assert L.ov2_map_merge_points_batch(ctx.h, 0, None, None, None, None, None, None, None) == 0
        assert call([dm.h], [0, 0]) == 0 and same_tables(before, dm.download())   # an empty list
        assert call([dm.h], [0, n]) == 0 and not same_tables(before, dm.download())   # and the map still works
    finally:
        dm.close(); other.close()


def test_asynchronous_form(ctx):
    key = MAPS[1]
    pairs, cur, _ = full_list(*key)
    dm, twin = fresh(ctx, key), fresh(ctx, key)
    try:
        assert DM.merge_points_batch(ctx, [dm], [pairs], [cur], want_header=False) is None   # out = NULL, pair_status = NULL: OV2_OK
        ctx.synchronize()
        DM.merge_points_batch(ctx, [twin], [pairs], [cur])
        assert same_tables(dm.download(), twin.download())
    finally:
        dm.close(); twin.close()
