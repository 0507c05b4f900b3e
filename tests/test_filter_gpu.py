"""Keyframe culling on the GPU side (Estimator::mapFiltering, reference src/estimator.cpp:101-183): the C++ host stage
against the checker (tests/filter_ref.py), the batched device form ov2_map_filter_keyframes_batch against the host stage --
lists, counts and the whole canonical state of the tables, exactly: only index work is involved --, batches, capacity
growth, saved states, refusals, and the closed loop with the stage switched on.
Maps: synth_filter.make_map, (keyframes, landmarks) in {(21, 60), (24, 200), (40, 1200)} at the ratios 0.9f and 0.95f,
nmin_covscore 25.  21 keyframes is the fewest that pass the kfid >= 20 gate; the three sizes put 1, 2 and ~25 workgroups of
rows behind every scan, and the largest gives the walk keyframes with more rows than its workgroup has lanes."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, host_map, synth_filter
import filter_ref as R
from test_filter_ref_cpu import CASES, RATIOS, assert_host_equals_checker

pytestmark = pytest.mark.gpu
INVALID = -1   # OV2_ERR_INVALID (include/ov2slam_hip.h)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


_maps = {}


def the_map(nk, nl, seed=None):
    key = (nk, nl, nk if seed is None else seed)
    if key not in _maps:
        _maps[key] = synth_filter.make_map(nk, nl, seed=key[2])
    return _maps[key]


_host = {}


def host_result(ctx, nk, nl, ratio, seed=None):
    """the host stage on the map, once per case: (removed, stats, unset3d lmids, canonical state of a mirror attached to the
    FILTERED host map)"""
    key = (nk, nl, ratio, seed)
    if key not in _host:
        m = the_map(nk, nl, seed)
        hm, ref = assert_host_equals_checker(m, ratio)
        hm.attach_device(ctx)
        state = DM.canonical_state(_Borrowed(ctx, hm.device_handle()).download())
        _host[key] = (ref["removed"], dict(candidates=ref["candidates"], few3d=ref["few3d"]), sorted(ref["unset3d"]), state)
        del hm
    return _host[key]


class _Borrowed:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.lib, h
        self._p = DM.DeviceMap._p
        self.download = lambda: DM.DeviceMap.download(self)


def assert_device_equals_host(res, dm, host):
    removed, st, unset, state = host
    assert res["removed"] == removed
    assert dict(candidates=res["candidates"], few3d=res["few3d"]) == st
    assert res["unset3d"] == unset
    assert DM.canonical_state(dm.download()) == state


@pytest.mark.parametrize("nk,nl", CASES)
@pytest.mark.parametrize("ratio", RATIOS)
def test_host_stage_equals_checker_and_device_form_equals_host_stage(ctx, nk, nl, ratio):
    host = host_result(ctx, nk, nl, ratio)
    assert len(host[0]) >= 3 and host[1]["few3d"] >= 1 and len(host[2]) >= 16
    dm = DM.DeviceMap.from_filter_map(ctx, the_map(nk, nl))
    try:
        res = dm.filter_keyframes_batch(nmin_covscore=25, ratio=ratio)[0]
        assert_device_equals_host(res, dm, host)
    finally:
        dm.close()


def test_batch_of_eight_equals_eight_single_calls(ctx):
    """eight distinct maps in one call, one of them with newkf < 20 (gated: zero header, tables untouched); and a call with
    the ratio 1.0, which is the stage switched off"""
    shapes = [(21, 60, 1), (24, 200, 2), (40, 1200, 3), (22, 90, 4), (30, 400, 5), (21, 64, 6), (26, 300, 7), (23, 128, 8)]
    maps = [DM.DeviceMap.from_filter_map(ctx, the_map(*s)) for s in shapes]
    gated = 3
    newkf = [m.newkf for m in maps]
    newkf[gated] = 19
    try:
        before = DM.canonical_state(maps[gated].download())
        off = DM.filter_keyframes_batch(ctx, maps[:2], ratio=1.0)
        assert off == [dict(candidates=0, few3d=0, removed=[], unset3d=[])] * 2
        res = DM.filter_keyframes_batch(ctx, maps, newkf=newkf, ratio=0.9)
        assert res[gated] == dict(candidates=0, few3d=0, removed=[], unset3d=[])
        assert DM.canonical_state(maps[gated].download()) == before
        for b, s in enumerate(shapes):
            if b == gated:
                continue
            one = DM.DeviceMap.from_filter_map(ctx, the_map(*s))
            try:
                assert one.filter_keyframes_batch(ratio=0.9)[0] == res[b], s
                assert DM.canonical_state(one.download()) == DM.canonical_state(maps[b].download()), s
            finally:
                one.close()
            if s[2] <= 3:   # (these three are also checked against the host stage)
                assert_device_equals_host(res[b], maps[b], host_result(ctx, s[0], s[1], 0.9, seed=s[2]))
    finally:
        for m in maps:
            m.close()


def _setup_problem(ctx, dm):
    v = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)[0]
    f = DM.fetch_view(ctx, v, True)
    if f["aborted"]:
        return "aborted"
    keys = sorted(zip(f["res_type"].tolist(), f["res_kfid"].tolist(), f["res_lmid"].tolist(), f["res_uv"][:, 0].tolist(), f["res_uv"][:, 1].tolist()))
    return keys, dict(zip(f["pose_kfid"].tolist(), f["pose_const"].tolist())), f["bad_lmid"].tolist()


def test_filter_after_the_tables_grew_and_setup_after_the_filter(ctx):
    """a map created at the tightest capacity grows past every capacity while its keyframes come in (the stage's scratch
    arrays follow, ensure_capacity), is filtered, squeezed and set up: same lists, same tables, same local-BA problem as a
    mirror of the filtered host map gives"""
    nk, nl, ratio = 40, 1200, 0.9
    m = the_map(nk, nl)
    host = host_result(ctx, nk, nl, ratio)
    dm = DM.DeviceMap.from_filter_map(ctx, m, capacity=(1, 1, 1))
    hm = host_map.FilterMap(m)
    try:
        assert dm.rows()[1] >= len(m["obs_kf"]) > 1
        res = dm.filter_keyframes_batch(ratio=ratio)[0]
        assert_device_equals_host(res, dm, host)
        before, after = dm.compact()
        assert after < before and DM.canonical_state(dm.download()) == host[3]
        hm.map_filtering(ratio=ratio)
        hm.attach_device(ctx)
        ref = _Borrowed(ctx, hm.device_handle())
        ref.newkf = m["newkf"]
        a, b = _setup_problem(ctx, dm), _setup_problem(ctx, ref)
        assert a == b and a != "aborted" and len(a[0]) > 100
    finally:
        dm.close()
        del hm


def test_save_filter_restore_filter_and_update_refused(ctx):
    nk, nl, ratio = 24, 200, 0.9
    host = host_result(ctx, nk, nl, ratio)
    dm = DM.DeviceMap.from_filter_map(ctx, the_map(nk, nl))
    try:
        start = DM.canonical_state(dm.download())
        dm.save_state()
        first = dm.filter_keyframes_batch(ratio=ratio)[0]
        assert_device_equals_host(first, dm, host)
        DM.restore_state_batch(ctx, [dm])
        assert DM.canonical_state(dm.download()) == start
        again = dm.filter_keyframes_batch(ratio=ratio)[0]
        assert again == first
        assert DM.canonical_state(dm.download()) == host[3]
        # set-up -> filter: the set-up can no longer be updated from, as after a squeeze.  (The set-up itself clears is3d_ of
        # the bad landmarks in its window, as Optimizer::localBA does, so this third call is not compared with the first.)
        views = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)
        hs = (C.c_void_p * 1)(dm.h)
        outl = (C.c_void_p * 1)(None if views[0].aborted else views[0].res_outlier)
        dm.filter_keyframes_batch(ratio=ratio)
        assert ctx.lib.ov2_map_local_ba_update_batch(ctx.h, 1, hs, outl, None, None) == INVALID
    finally:
        dm.close()


def test_refusals_leave_the_tables_alone(ctx):
    m = the_map(21, 60)
    dm, other = DM.DeviceMap.from_filter_map(ctx, m), DM.DeviceMap.from_filter_map(ctx, m)
    try:
        ctx.lib.ov2_map_remove_keyframe(dm.h, 7)
        before, before_other = DM.canonical_state(dm.download()), DM.canonical_state(other.download())
        L, out = ctx.lib, (DM.FilterC * 2)()
        call = lambda hs, nk, o: L.ov2_map_filter_keyframes_batch(ctx.h, len(hs), (C.c_void_p * len(hs))(*hs),
                                                                    np.array(nk, np.int32).ctypes.data_as(C.c_void_p), 25, 0.9, o)
        assert call([dm.h], [7], out) == INVALID                          # a dead new keyframe
        assert call([dm.h], [m["n_kf"] + 100], out) == INVALID            # ... or one beyond the table
        assert call([other.h, dm.h, other.h], [20, 20, 20], (DM.FilterC * 3)()) == INVALID   # a map listed twice
        assert call([dm.h], [20], None) == INVALID                        # nowhere to report to
        assert DM.canonical_state(dm.download()) == before
        assert DM.canonical_state(other.download()) == before_other
        assert call([dm.h], [20], out) == 0 and out[0].n_removed >= 3     # and the map still works
    finally:
        dm.close(); other.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------
N_FRAMES, KF_EVERY = 200, 5


@pytest.fixture(scope="module")
def frames():
    """the 200 left images, and the right image of every keyframe (the loop reads no other)"""
    from ov2slam_amd import synth_scene
    sc = synth_scene.PlaneScene(N_FRAMES)
    left = [sc.left(t) for t in range(N_FRAMES)]
    right = {t: sc.right(t) for t in range(0, N_FRAMES, KF_EVERY)}
    return sc, left, right


def _loop(ctx, frames, ratio):
    """the fixed keyframe cadence of test_cpp_loop_matches_the_python_loop (a keyframe every 5 frames) with the reference's
    covisibility local BA on the device map mirror"""
    from ov2slam_amd import synth_scene
    sc, left, right = frames
    cl = host_map.CppSlam(ctx, synth_scene.K4, synth_scene.BASELINE, synth_scene.W, synth_scene.H, policy="slam_loop", kf_every=KF_EVERY,
                          ba_window=0, device_map=True)
    if ratio is not None:
        cl.set_kf_filtering(ratio)
    try:
        for t in range(N_FRAMES):
            cl.step(0.05 * t, left[t], right.get(t, left[t]))
        host = cl.export_map()
        cl.flush_device()
        dev = DM.canonical_state(_Borrowed(ctx, cl.device_handle()).download())
    finally:
        cl.close()
    return np.array(cl.traj), getattr(cl, "filter_stats", None), host, dev


def test_closed_loop_with_keyframe_culling(ctx, frames):
    """200 frames of the plane scene, a keyframe every 5 frames, kf_filtering_ratio 0.9: no frame ends the loop, keyframes
    are removed after keyframe 20, the trajectory stays within the bound of the other loop tests, the device mirror equals
    the host map at the end, two runs are bit-identical, and the ratio left at 1 is the unfiltered loop bit for bit."""
    from ov2slam_amd import slam_loop
    sc = frames[0]
    traj, fs, host, dev = _loop(ctx, frames, 0.9)
    assert len(traj) == N_FRAMES and len(fs) == N_FRAMES // KF_EVERY
    removed = [k for s in fs for k in s["removed"]]
    print("removed keyframes (ids, at most 11 listed per keyframe):", removed, "removed per keyframe:", [s["n_removed"] for s in fs],
          "candidates per keyframe:", [s["candidates"] for s in fs])
    assert all(not s["ran"] for s in fs[:20]) and all(s["ran"] for s in fs[20:])
    assert len(removed) >= 1
    gt = [sc.pose(t) for t in range(N_FRAMES)]
    ate = slam_loop.ate_rmse(list(traj), gt)
    print("ATE with culling: %.5f m" % ate)
    assert ate < 0.01
    kf_h, lm_h, ob_h = host
    kf_d, lm_d, ob_d = dev
    assert not set(removed) & set(kf_h)
    assert sorted(kf_h) == sorted(kf_d) and all(np.allclose(kf_h[k], kf_d[k], atol=1e-12) for k in kf_h)
    assert sorted(lm_h) == sorted(lm_d)
    assert set(ob_h) == set(ob_d) and all(bool(ob_h[o]) == bool(ob_d[o]) for o in ob_h)
    traj2 = _loop(ctx, frames, 0.9)[0]
    assert np.array_equal(traj.view(np.uint64), traj2.view(np.uint64))
    plain, off = _loop(ctx, frames, None)[0], _loop(ctx, frames, 1.0)[0]
    assert np.array_equal(plain.view(np.uint64), off.view(np.uint64))
    assert not np.array_equal(plain.view(np.uint64), traj.view(np.uint64))
