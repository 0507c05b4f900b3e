"""ov2_map_local_pose_graph_batch (csrc/map.hip, csrc/posegraph.hip): Optimizer::localPoseGraph (reference
src/optimizer.cpp:2346-2592) on mirror-only maps -- assembly, solve, degenerate gate and update enqueued on one stream --
against the C++ host stage (Optimizer::localPoseGraph with a mirror attached, flushed).

Maps: synth_filter.make_map at (21, 60) and (40, 1200) with eight more 3D landmarks that only the three newest keyframes see
(with_younger, a local copy of the helper of test_map_pg_update_gpu.py), so that the younger branch of the update has work;
the new keyframe is nk - 4.  The strided map is make_map(300, 60) itself (it takes a fraction of a second): its chain 5 .. 296
lists 292 poses, so the assembly, the solver's pose / edge loops and the update's keyframe scan all go past 256.
newTwc: the stored pose of newkf times se3_exp of a twist of norm 0.05.

Bar against the host stage: every integer and state column exact, poses and points BITWISE equal, the solve's final cost and
iteration count equal to the host's last_pg_."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import expm

import loop_close_ref as R
from ov2slam_amd import device_map as DM, host_map, synth_filter
from test_oracle_pg import hat6

pytestmark = pytest.mark.gpu
SHAPES = [(21, 60), (40, 1200)]
K4 = synth_filter.K4


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def with_younger(m, n_extra=8):
    """a copy of the map with n_extra more 3D landmarks, seen by the three newest keyframes only"""
    nk, nl = m["n_kf"], m["n_lm"]
    rng = np.random.default_rng(1000 + nk)
    kf, lm = [], []
    for i in range(n_extra):
        a = nk - 3 + i % 3
        kf.append(a); lm.append(nl + i)
        if a != nk - 1:
            kf.append(nk - 1); lm.append(nl + i)
    obs_kf = np.concatenate([m["obs_kf"], np.array(kf, np.int32)])
    obs_lm = np.concatenate([m["obs_lm"], np.array(lm, np.int32)])
    uv = np.stack([rng.uniform(8, m["w"] - 8, len(kf)), rng.uniform(8, m["h"] - 8, len(kf))], 1).astype(np.float32)
    obs_uv = np.concatenate([m["obs_uv"], uv])
    o = np.lexsort((obs_lm, obs_kf))
    one = np.ones(n_extra, np.uint8)
    X = np.stack([rng.uniform(-2, 2 + 0.1 * nk, n_extra), rng.uniform(-1.5, 1.5, n_extra), rng.uniform(2, 9, n_extra)], 1)
    return dict(m, n_lm=nl + n_extra, obs_kf=obs_kf[o], obs_lm=obs_lm[o], obs_uv=obs_uv[o],
                lm_3d=np.concatenate([m["lm_3d"], one]), lm_kp3d=np.concatenate([m["lm_kp3d"], one]),
                lm_isobs=np.concatenate([m["lm_isobs"], one]), lm_xyz=np.vstack([m["lm_xyz"], X]))


_maps = {}


def the_map(nk, nl, seed=None):
    key = (nk, nl, nk if seed is None else seed)
    if key not in _maps:
        _maps[key] = with_younger(synth_filter.make_map(nk, nl, seed=key[2]))
    return _maps[key]


def twisted(m, newkf, seed=0, norm=0.05):
    """the stored pose of newkf times se3_exp of a twist of the given norm"""
    v = np.random.default_rng(77 + seed).normal(0, 1, 6)
    return R.pose7(R.mat(m["poses"][newkf]) @ expm(hat6(v / np.linalg.norm(v) * norm)))


def shifted(m, newkf, metres):
    p = np.array(m["poses"][newkf], np.float64)
    p[1] += metres
    return p


class _Borrowed:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.lib, h
        self._p = DM.DeviceMap._p
        self.download = lambda: DM.DeviceMap.download(self)


def _bits(state):
    """canonical state with every double as its bit pattern: == is then bitwise (0.0 vs -0.0, NaN)"""
    kfs, lms, obs = state
    b = lambda t: tuple(np.asarray(t, np.float64).view(np.uint64).tolist())
    return {k: b(v) for k, v in kfs.items()}, {l: (b(p), s) for l, (p, s) in lms.items()}, obs


def _raw_tables(d):
    """every downloaded table as bytes: == is then 'the mirror is bitwise unchanged'"""
    return {k: v.tobytes() for k, v in d.items()}


def host_stage(ctx, m, newkf, loop, Tn, stereo=True, dead=()):
    """(accepted, final cost, n_log, canonical state of the flushed mirror) of Optimizer::localPoseGraph on the host map"""
    hm = host_map.FilterMap(m, stereo=stereo)
    for k in dead:
        hm.remove_keyframe(k)
    hm.attach_device(ctx)
    hm.set_cur_frame(None)      # the constructor leaves a keyframe OBJECT standing in as the current frame: it would move twice
    ok, fc, nlog = hm.local_pose_graph(ctx, newkf, loop, Tn)
    hm.flush_device()
    state = DM.canonical_state(_Borrowed(ctx, hm.device_handle()).download())
    del hm
    return ok, fc, nlog, state


def fresh(ctx, m, dead=()):
    dm = DM.DeviceMap.from_filter_map(ctx, m)
    for k in dead:
        dm.remove_keyframe(k)
    return dm


def assert_same_state(host, dev, tag):
    hk, hl, ho = host
    dk, dl, do = dev
    assert set(hk) == set(dk) and set(hl) == set(dl) and ho == do, tag                  # integer columns
    assert {l: s for l, (_, s) in hl.items()} == {l: s for l, (_, s) in dl.items()}, tag  # landmark states
    dpose = max(np.abs(np.array(hk[k]) - np.array(dk[k])).max() for k in hk)
    dpt = max(np.abs(np.array(hl[l][0]) - np.array(dl[l][0])).max() for l in hl)
    print(f"[local_pg {tag}] max |pose diff| {dpose:.3e}, max |point diff| {dpt:.3e}")
    assert _bits(host) == _bits(dev), tag


@pytest.mark.parametrize("nk,nl", SHAPES)
def test_whole_statement_equals_host_stage(ctx, nk, nl):
    """Largest difference measured on these two maps: 0 (bitwise), poses and points."""
    m = the_map(nk, nl)
    newkf, loop = nk - 4, 5
    Tn = twisted(m, newkf)
    ok, fc, nlog, host = host_stage(ctx, m, newkf, loop, Tn)
    assert ok == 1 and nlog >= 2
    dm = fresh(ctx, m)
    try:
        before = dm.download()
        r = dm.local_pose_graph_batch(newkf=[newkf], kfloop_id=[loop], newTwc=[Tn])[0]
        after = dm.download()
    finally:
        dm.close()
    assert r["verdict"] == DM.LPG_DONE and r["kfloop_id"] == loop and r["n_pose"] == newkf - loop + 1
    assert r["n_kf_chain"] == newkf - loop and r["n_kf_younger"] == 3 and r["n_lm_moved"] > 5
    assert (r["result"].final_cost, r["result"].n_log) == (fc, nlog)
    assert r["result"].final_cost < r["result"].initial_cost
    assert_same_state(host, DM.canonical_state(after), f"{nk},{nl}")
    for k in range(loop + 1):       # the loop keyframe and everything below it: bit-unchanged
        assert np.array_equal(before["kf_pose"][k].view(np.uint64), after["kf_pose"][k].view(np.uint64))
    # T_corr is opt * inverse(old(newkf)): it carries the old pose of newkf onto the new one
    got = R.mat(r["T_corr"]) @ R.mat(before["kf_pose"][newkf])
    assert np.abs(got - R.mat(after["kf_pose"][newkf])).max() <= 1e-12


def test_assembly_equals_host_hook(ctx):
    """the assembled device block against Optimizer::assembleLocalPoseGraph, bitwise: a plain chain, dead keyframes inside
    the range with a dead kfloop_id, a two-pose chain, and the big map"""
    cases = [((21, 60), (), 17, 5), ((21, 60), (5, 6, 9, 12), 17, 5), ((21, 60), (), 17, 16), ((40, 1200), (7,), 36, 3)]
    for shape, dead, newkf, loop in cases:
        m = the_map(*shape)
        Tn = twisted(m, newkf, seed=loop)
        hm = host_map.FilterMap(m)
        for k in dead:
            hm.remove_keyframe(k)
        want = hm.assemble_local_pose_graph(newkf, loop, Tn)
        del hm
        dm = fresh(ctx, m, dead)
        try:
            got = DM.local_pose_graph_assemble(ctx, [dm], [newkf], [loop], [Tn])[0]
        finally:
            dm.close()
        assert want is not None and got is not None
        assert got["kfids"].tolist() == want["kfids"].tolist() and len(want["kfids"]) >= 2
        assert np.array_equal(got["pose"].view(np.uint64), want["pose"].view(np.uint64)), (shape, dead)
        assert np.array_equal(got["T_ij"].view(np.uint64), want["T_ij"].view(np.uint64)), (shape, dead)
        assert want["edge_i"].tolist() == list(range(len(want["kfids"]) - 1)) + [0]      # the edge order the device block uses
        if dead == (5, 6, 9, 12):      # the dead kfloop_id walked up, the dead keyframes of the range are not listed
            assert got["kfids"].tolist() == [7, 8, 10, 11, 13, 14, 15, 16, 17]


_degenerate = {}


def degenerate_input(ctx, m, newkf):
    """(loop keyframe, newTwc) on which the host stage refuses the solution: the stored pose moved by 2 m, or further until it
    does -- a precondition on the input, not a tolerance on the code"""
    key = (m["n_kf"], m["n_lm"], newkf, float(m["poses"][newkf][1]))
    if key not in _degenerate:
        loop = newkf - 3
        for metres in (2.0, 4.0, 8.0):
            Tn = shifted(m, newkf, metres)
            if host_stage(ctx, m, newkf, loop, Tn, stereo=True)[0] == 0:
                _degenerate[key] = (loop, Tn)
                break
        else:
            raise AssertionError("the host stage accepts every offset tried")
    return _degenerate[key]


def test_degenerate_gate(ctx):
    m = the_map(21, 60)
    newkf = 17
    loop, Tn = degenerate_input(ctx, m, newkf)
    assert host_stage(ctx, m, newkf, loop, Tn, stereo=True)[0] == 0
    dm = fresh(ctx, m)
    try:
        before = dm.download()
        d_n = ctx.to_device(np.array([7], np.int32))
        r = dm.local_pose_graph_batch(newkf=[newkf], kfloop_id=[loop], newTwc=[Tn], stereo=True, d_n_pairs=d_n)[0]
        assert r["verdict"] == DM.LPG_DEGENERATE and r["n_pose"] == 4 and r["kfloop_id"] == loop
        assert (r["n_kf_chain"], r["n_kf_younger"], r["n_lm_moved"]) == (0, 0, 0) and not r["T_corr"].any()
        assert r["result"].n_log >= 2          # the solve ran; only its result was refused
        assert _raw_tables(dm.download()) == _raw_tables(before)
        assert d_n.get().tolist() == [0]
    finally:
        dm.close()
    # the same input as mono: accepted, and equal to the host stage run as mono
    ok, fc, nlog, host = host_stage(ctx, m, newkf, loop, Tn, stereo=False)
    assert ok == 1
    dm = fresh(ctx, m)
    try:
        d_n = ctx.to_device(np.array([7], np.int32))
        r = dm.local_pose_graph_batch(newkf=[newkf], kfloop_id=[loop], newTwc=[Tn], stereo=False, d_n_pairs=d_n)[0]
        assert r["verdict"] == DM.LPG_DONE and (r["result"].final_cost, r["result"].n_log) == (fc, nlog)
        assert d_n.get().tolist() == [7]
        assert_same_state(host, DM.canonical_state(dm.download()), "mono")
    finally:
        dm.close()


@pytest.mark.parametrize("dead,loop", [((17,), 5), ((15, 16), 15)], ids=["dead_newkf", "walk_finds_nothing"])
def test_no_chain(ctx, dead, loop):
    m = the_map(21, 60)
    dm = fresh(ctx, m, dead)
    try:
        before = dm.download()
        d_n = ctx.to_device(np.array([7], np.int32))
        r = dm.local_pose_graph_batch(newkf=[17], kfloop_id=[loop], newTwc=[twisted(m, 17)], d_n_pairs=d_n)[0]
        assert r["verdict"] == DM.LPG_NO_CHAIN and r["kfloop_id"] == -1 and r["n_pose"] == 0
        assert (r["n_kf_chain"], r["n_kf_younger"], r["n_lm_moved"]) == (0, 0, 0) and not r["T_corr"].any()
        assert _raw_tables(dm.download()) == _raw_tables(before)
        assert d_n.get().tolist() == [0]
    finally:
        dm.close()


def _batch_jobs(ctx):
    """eight maps with different seeds: chains of 2, 4 and about 30 poses, the three verdicts mixed (all under stereo = 1)"""
    shapes = [(21, 60, 1), (24, 200, 2), (40, 1200, 3), (22, 90, 4), (30, 400, 5), (21, 64, 6), (26, 300, 7), (23, 128, 8)]
    jobs = []
    for i, (nk, nl, seed) in enumerate(shapes):
        m = the_map(nk, nl, seed)
        newkf = nk - 4
        kind = ("two", "four", "long", "degenerate", "dead_newkf", "four", "degenerate", "walk")[i]
        dead, loop, Tn, want = (), 5, twisted(m, newkf, seed), DM.LPG_DONE
        if kind == "two":
            loop = newkf - 1
        elif kind == "four":
            loop = newkf - 3
        elif kind == "degenerate":
            loop, Tn = degenerate_input(ctx, m, newkf)
            want = DM.LPG_DEGENERATE
        elif kind == "dead_newkf":
            dead, want = (newkf,), DM.LPG_NO_CHAIN
        elif kind == "walk":
            dead, loop, want = (newkf - 2, newkf - 1), newkf - 2, DM.LPG_NO_CHAIN
        jobs.append(dict(m=m, newkf=newkf, loop=loop, Tn=Tn, dead=dead, want=want))
    return jobs


def test_batch_of_eight_equals_eight_single_calls(ctx):
    jobs = _batch_jobs(ctx)
    B = len(jobs)
    singles = []
    ctx.kernel_timing(True)
    try:
        for j in jobs:
            dm = fresh(ctx, j["m"], j["dead"])
            try:
                ctx.kernel_times()
                r = dm.local_pose_graph_batch(newkf=[j["newkf"]], kfloop_id=[j["loop"]], newTwc=[j["Tn"]])[0]
                t = ctx.kernel_times()
                singles.append((r, _bits(DM.canonical_state(dm.download())), t))
            finally:
                dm.close()
            assert r["verdict"] == j["want"]
        assert sorted(r["n_pose"] for r, _, _ in singles) == [0, 0, 2, 4, 4, 4, 4, 32]
        for order in (list(range(B)), list(range(B))[::-1]):
            maps = [fresh(ctx, jobs[k]["m"], jobs[k]["dead"]) for k in order]
            try:
                ctx.kernel_times()
                res = DM.local_pose_graph_batch(ctx, maps, [jobs[k]["newkf"] for k in order], [jobs[k]["loop"] for k in order],
                                                [jobs[k]["Tn"] for k in order])
                t = ctx.kernel_times()
                for slot, k in enumerate(order):
                    assert res[slot]["raw"] == singles[k][0]["raw"], (order, k)
                    assert _bits(DM.canonical_state(maps[slot].download())) == singles[k][1], (order, k)
            finally:
                for dm in maps:
                    dm.close()
            # the launch count does not depend on B: assembly, gate, the four of the update and the gather; one minimiser
            one = singles[0][2]
            assert {n: c for n, (_, c) in t.items()} == {n: c for n, (_, c) in one.items()} == \
                {"map_setup_kernels": 7, "pose_graph_kernel": 1}
    finally:
        ctx.kernel_timing(False)


def test_strided_paths(ctx):
    """300 keyframes, 60 landmarks from make_map itself; the chain 5 .. 296 lists 292 poses"""
    m = with_younger(synth_filter.make_map(300, 60, seed=300))
    newkf, loop = 296, 5
    Tn = twisted(m, newkf)
    ok, fc, nlog, host = host_stage(ctx, m, newkf, loop, Tn)
    assert ok == 1
    dm = fresh(ctx, m)
    try:
        g = DM.local_pose_graph_assemble(ctx, [dm], [newkf], [loop], [Tn])[0]
        r = dm.local_pose_graph_batch(newkf=[newkf], kfloop_id=[loop], newTwc=[Tn])[0]
        after = DM.canonical_state(dm.download())
    finally:
        dm.close()
    assert len(g["kfids"]) == 292 >= 258 and r["n_pose"] == 292 and r["verdict"] == DM.LPG_DONE and r["n_kf_chain"] == 291
    assert (r["result"].final_cost, r["result"].n_log) == (fc, nlog)
    assert_same_state(host, after, "300,60")


def _pairs_of(m, n=6):
    """n disjoint (prev, new) pairs among the observed 3D landmarks of the map"""
    seen = np.unique(m["obs_lm"])
    ok = seen[(m["lm_3d"][seen] != 0) & (m["lm_kp3d"][seen] != 0)]
    assert len(ok) >= 2 * n
    return np.stack([ok[1:2 * n:2], ok[0:2 * n:2]], 1).astype(np.int32)


def test_async_form_chains_into_merge_and_structure_ba(ctx):
    """out == NULL with d_n_pairs, then merge_points_batch_dev and structure_ba_batch_dev on the same stream, one
    synchronisation at the end == the three stages in their host-pointer forms with a synchronisation after each.  Map 0 is
    DONE and merges its pairs, map 1 is DEGENERATE and merges none."""
    ms = [the_map(24, 200, 2), the_map(21, 60)]
    newkf = [20, 17]
    loop1, T1 = degenerate_input(ctx, ms[1], 17)
    loops, Ts = [5, loop1], [twisted(ms[0], 20), T1]
    pairs = [_pairs_of(ms[0]), _pairs_of(ms[1])]
    cam = DM.SbaCamC()
    cam.calib_l[:], cam.calib_r[:], cam.T_rl[:] = list(K4), list(K4), [-0.11, 0, 0, 0, 0, 0, 1.0]
    maps, twins = [fresh(ctx, m) for m in ms], [fresh(ctx, m) for m in ms]
    try:
        off = np.array([0, len(pairs[0]), len(pairs[0]) + len(pairs[1])], np.int32)
        flat = np.concatenate(pairs)
        d_prev, d_new = ctx.to_device(flat[:, 0].copy()), ctx.to_device(flat[:, 1].copy())
        d_n = ctx.to_device(np.array([len(pairs[0]), len(pairs[1])], np.int32))
        d_st = ctx.to_device(np.full(len(flat), DM.MERGE_NOT_RUN, np.uint8))
        hs = (C.c_void_p * 2)(*[m.h for m in maps])
        assert DM.local_pose_graph_batch(ctx, maps, newkf, loops, Ts, d_n_pairs=d_n, want=False) is None
        assert ctx.lib.ov2_map_merge_points_batch_dev(ctx.h, 2, hs, off.ctypes.data_as(C.c_void_p), d_prev.ptr, d_new.ptr, None, d_n.ptr,
                                                      None, d_st.ptr) == 0
        assert DM.structure_ba_batch(ctx, maps, DM.DevIds(off, d_new, d_n), [cam, cam], dev=True, d_status=d_st, want_header=False) is None
        ctx.synchronize()
        assert d_n.get().tolist() == [len(pairs[0]), 0]
        # host-pointer forms on the twins, each synchronising
        r = DM.local_pose_graph_batch(ctx, twins, newkf, loops, Ts)
        assert [x["verdict"] for x in r] == [DM.LPG_DONE, DM.LPG_DEGENERATE]
        lists = [pairs[b] if r[b]["verdict"] == DM.LPG_DONE else np.zeros((0, 2), np.int32) for b in range(2)]
        hdr, st = DM.merge_points_batch(ctx, twins, lists)
        assert hdr[0]["n_merged"] == len(pairs[0]) and hdr[1]["n_pairs"] == 0
        h = DM.structure_ba_batch(ctx, twins, [lists[b][:, 1][st[b] == DM.MERGE_DONE] for b in range(2)], [cam, cam])
        assert h[0]["n_lm"] == len(pairs[0]) and h[1]["n_listed"] == 0
        for a, b in zip(maps, twins):
            assert _bits(DM.canonical_state(a.download())) == _bits(DM.canonical_state(b.download()))
        assert d_st.get()[:len(pairs[0])].tolist() == [DM.MERGE_DONE] * len(pairs[0])
    finally:
        for m in maps + twins:
            m.close()


def test_refusals(ctx):
    from ov2slam_amd import frontend
    m = the_map(21, 60)
    Tn = twisted(m, 17)
    dm = fresh(ctx, m)
    ctx2 = frontend.Context(0)
    foreign = DM.DeviceMap.from_filter_map(ctx2, m)
    try:
        before = _raw_tables(dm.download())
        with pytest.raises(Exception, match=r"\(-1\).*twice"):
            DM.local_pose_graph_batch(ctx, [dm, dm], [17, 17], [5, 5], [Tn, Tn])
        with pytest.raises(Exception, match=r"\(-1\).*another context"):
            DM.local_pose_graph_batch(ctx, [dm, foreign], [17, 17], [5, 5], [Tn, Tn])
        with pytest.raises(Exception, match=r"\(-1\).*null"):
            DM.local_pose_graph_batch(ctx, [dm], [17], [5], None)
        hs = (C.c_void_p * 1)(dm.h)
        nk, lo = np.array([17], np.int32), np.array([5], np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx.lib.ov2_map_local_pose_graph_batch(ctx.h, -1, hs, p(nk), p(lo), p(Tn), 1, None, None, None) == -1
        assert ctx.lib.ov2_map_local_pose_graph_batch(ctx.h, 0, None, None, None, None, 1, None, None, None) == 0
        ctx.synchronize()
        assert _raw_tables(dm.download()) == before
        # a valid call ends what the set-up made before it can be updated from
        view = DM.setup_batch(ctx, [dm], calib_l=K4)
        assert dm.local_pose_graph_batch(newkf=[17], kfloop_id=[5], newTwc=[Tn])[0]["verdict"] == DM.LPG_DONE
        with pytest.raises(Exception, match=r"\(-1\).*no set-up to update from"):
            DM.update_batch(ctx, [dm], view)
    finally:
        foreign.close()
        dm.close()
        ctx2.close()


def test_update_dev_form_with_skip_bytes(ctx):
    """ov2_map_pose_graph_update_batch_dev alone: poses in device memory == the host form; a set skip byte leaves the map alone"""
    m = the_map(21, 60)
    ids = np.arange(6, 18, dtype=np.int32)
    T = np.stack([twisted(m, int(k), seed=int(k), norm=0.01) for k in ids])
    a, b, c = fresh(ctx, m), fresh(ctx, m), fresh(ctx, m)
    try:
        want = a.pose_graph_update_batch(newkf=[17], chain_kfid=[ids], chain_Twc=[T])[0]
        before = _raw_tables(c.download())
        d_T = ctx.to_device(np.concatenate([T, T]))
        d_skip = ctx.to_device(np.array([0, 1], np.uint8))
        got = DM.pose_graph_update_batch_dev(ctx, [b, c], [17, 17], [ids, ids], d_T, d_skip)
        assert got[0]["n_lm_moved"] == want["n_lm_moved"] > 5 and got[0]["n_kf_chain"] == len(ids)
        assert np.array_equal(got[0]["T_corr"].view(np.uint64), want["T_corr"].view(np.uint64))
        # (two mirrors are compared by their live entries: the spare slots of a table hold whatever the allocation held)
        assert _bits(DM.canonical_state(a.download())) == _bits(DM.canonical_state(b.download()))
        assert (got[1]["n_kf_chain"], got[1]["n_kf_younger"], got[1]["n_lm_moved"]) == (0, 0, 0) and not got[1]["T_corr"].any()
        assert _raw_tables(c.download()) == before
    finally:
        for dm in (a, b, c):
            dm.close()
