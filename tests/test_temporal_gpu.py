"""Temporal triangulation (Mapper::triangulateTemporal, reference src/mapper.cpp:191-344) on the GPU: the host stage
(ov2::SlamManager::triangulateTemporal: selection + bookkeeping around one ov2_triangulate_pairs call) against the checker
tests/temporal_ref.py; the batched device form on the map mirror (ov2_map_triangulate_temporal_batch) against the host
stage; the device form between the set-up and the update of a local BA; and the closed loop with the stage switched on,
on a stream whose right image hides a stripe from the stereo matcher.

Maps: ov2slam_amd/synth_temporal.py, sizes and seeds temporal_ref.GPU_CASES (tests/test_temporal_ref_cpu.py shows that no
keypoint of them stands within 1e-6 of a threshold).  Bars: world point and inverse depth within 1e-8 m of the checker --
rounding of Tcicj at a few 1e-16, amplified by (z/b)^2 z <= 200^2 * 10 for depths <= 10 m and baselines >= 5 cm, gives
about 2e-10 m; 1e-8 is the bar of the P3P stage and leaves margin.  Pairs outside that conditioning (the 5 mm pair, with
stereo off) are compared on the branch they take."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, host_map, local_ba, slam_loop, synth_ba, synth_scene, synth_temporal

import temporal_ref as TR

pytestmark = pytest.mark.gpu

TOL = 1e-8
MARGIN = 1e-6


class _Handle:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.lib, h
    _p = staticmethod(DM.DeviceMap._p)


def _download(ctx, h):
    return DM.canonical_state(DM.DeviceMap.download(_Handle(ctx, h)))


def _assert_states_close(ref, got, tol):
    kf_r, lm_r, ob_r = ref
    kf_g, lm_g, ob_g = got
    assert sorted(kf_r) == sorted(kf_g)
    for k in kf_r:
        assert np.allclose(kf_r[k], kf_g[k], rtol=0, atol=1e-13), k
    assert sorted(lm_r) == sorted(lm_g), "live landmarks differ"
    for l in lm_r:
        assert lm_r[l][1] == lm_g[l][1], (l, lm_r[l][1], lm_g[l][1])
        assert np.allclose(lm_r[l][0], lm_g[l][0], rtol=0, atol=tol), l
    assert ob_r == ob_g, "live observations / stereo flags differ"


def _tables(dm):
    """the downloaded tables for an exact comparison: the rows of slots that hold no keyframe or landmark are not defined
    (only their state byte is cleared when a map is created), so they are blanked"""
    d = dm.download()
    d["kf_pose"][d["kf_state"] == 0] = 0.0
    d["lm_xyz"][(d["lm_state"] & DM.LM_ALIVE) == 0] = 0.0
    return d


def _host_stage(ctx, m, stereo, attach=False):
    hm = host_map.TemporalMap(m, stereo=stereo)
    if attach:
        hm.attach_device(ctx)
    lmid, branch, stats = hm.triangulate_temporal(ctx, TR.MAX_REPROJ_ERR)
    return hm, lmid, branch, stats


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("nk,nl,seed", TR.GPU_CASES)
def test_host_stage_equals_the_checker(ctx, oracle, nk, nl, seed, stereo):
    """the same branch per keypoint, the same landmarks turned 3D at the same point and inverse depth, the same observations
    removed; the edits reach the device mirror through the dirty lists: after flushDevice() the mirror equals the host map"""
    m = synth_temporal.make_map(nk, nl, seed=seed)
    poses, kps, lms = synth_temporal.as_dicts(m)
    ref = TR.triangulate_temporal(oracle, poses, kps, lms, m["newkf"], m["K4"], stereo, TR.MAX_REPROJ_ERR)
    hm, lmid, branch, stats = _host_stage(ctx, m, stereo, attach=True)
    before_kps = set(kps[m["newkf"]])
    assert lmid.tolist() == [r["lmid"] for r in ref]
    close = [r for r in ref if r["margin"] < MARGIN]          # compared on everything but the gate's verdict
    assert len(close) <= 1e-3 * len(ref)
    skip = {r["lmid"] for r in close}
    worst = 0.0
    n_good = n_cmp = 0
    for r, b in zip(ref, branch):
        if r["lmid"] in skip:
            continue
        assert int(b) == r["branch"], (r["lmid"], TR.BRANCH_NAMES[int(b)], TR.BRANCH_NAMES[r["branch"]])
        if r["branch"] != TR.GOOD:
            continue
        n_good += 1
        xyz, nobs = hm.landmark(r["lmid"])
        if r["baseline"] >= 0.05 and r["pt_a"][2] <= 10.0:
            d = max(np.abs(xyz - r["wpt"]).max(), abs(hm.invdepth(r["lmid"]) - r["invdepth"]))
            worst = max(worst, d)
            n_cmp += 1
    print(f"[temporal] K={nk} L={nl} seed={seed} stereo={int(stereo)}: {len(ref)} keypoints, {stats}, "
          f"max |wpt, invdepth - checker| = {worst:.3e} over {n_cmp} points")
    assert worst <= TOL
    assert n_cmp > 20 and stats["kps2d"] == len(ref)
    if not skip:
        assert stats["good"] == n_good == sum(r["branch"] == TR.GOOD for r in ref)
        assert stats["removed"] == sum(r["branch"] in TR.REMOVES for r in ref)
        assert stats["candidates"] == sum(r["branch"] >= TR.GOOD for r in ref)
    # the map after the stage: 3D exactly the good ones, the new keyframe lost exactly the removed observations
    kf_h, lm_h, ob_h = hm.export()
    for r in ref:
        if r["lmid"] in skip or r["branch"] == TR.NO_MAPPOINT:
            continue
        was3d = r["branch"] == TR.ALREADY_3D
        assert bool(lm_h[r["lmid"]][1] & DM.LM_3D) == (r["branch"] == TR.GOOD or was3d), r
    gone = {l for l in before_kps if (m["newkf"], l) not in ob_h and l in lm_h}
    assert gone - skip == {r["lmid"] for r in ref if r["branch"] in (TR.BEHIND_REMOVED, TR.REPROJ_REMOVED)} - skip
    hm.flush_device()
    _assert_states_close((kf_h, lm_h, ob_h), _download(ctx, hm.device_handle()), 0.0)


def _device_map_of(ctx, m):
    return DM.DeviceMap.from_temporal_map(ctx, m)


def _expected(ctx, m, stereo):
    hm, lmid, branch, stats = _host_stage(ctx, m, stereo)
    good = lmid[branch == TR.GOOD]
    removed = lmid[np.isin(branch, TR.REMOVES)]
    # the mirror keeps one 3D flag per landmark for its keypoints (lm_state_of): a 2D keypoint of a 3D map point, which the
    # reference skips with "should not happen" (:250-252), is not offered there
    stats = dict(stats, kps2d=stats["kps2d"] - int((branch == TR.ALREADY_3D).sum()))
    return hm, good, removed, stats


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("nk,nl,seed", TR.GPU_CASES)
def test_device_form_equals_the_host_stage(ctx, nk, nl, seed, stereo):
    """the same maps without their dangling references (keypoints without a map point, observers without a keyframe or a
    keypoint: the mirror has no way to hold them, an observation is live there only with both ends), one call with B = 1"""
    m = synth_temporal.make_map(nk, nl, seed=seed, dangling=False)
    hm, good, removed, stats = _expected(ctx, m, stereo)
    dm = _device_map_of(ctx, m)
    start = DM.canonical_state(dm.download())
    _assert_states_close(host_map.TemporalMap(m, stereo=stereo).export(), start, 0.0)   # the two builders agree
    out = dm.triangulate_temporal_batch(calib_l=m["K4"], stereo=stereo, max_reproj_err=TR.MAX_REPROJ_ERR)[0]
    assert out["selected"] == stats["kps2d"] and out["candidates"] == stats["candidates"]
    assert out["good_lmid"].tolist() == good.tolist() and len(good) > 10
    assert out["removed_lmid"].tolist() == removed.tolist() and len(removed) > 0
    _assert_states_close(hm.export(), DM.canonical_state(dm.download()), TOL)
    for l, w, rho in zip(out["good_lmid"], out["good_wpt"], out["good_invdepth"]):
        xyz, _ = hm.landmark(int(l))
        if np.linalg.norm(m["poses"][m["newkf"], :3] - m["poses"][_oldest(m, l), :3]) >= 0.05:
            assert np.abs(xyz - w).max() <= TOL and abs(hm.invdepth(int(l)) - rho) <= TOL, l
    dm.close()


def _oldest(m, l):
    return int(m["obs_kf"][m["obs_lm"] == l].min())


def test_batch_of_eight_equals_eight_single_calls(ctx):
    """B = 8 distinct maps in one call == eight B = 1 calls, exactly: tables after the call and the output lists; the
    asynchronous form (no lists) leaves the same tables; refusals leave the tables untouched"""
    specs = [(4, 300, 21), (12, 4000, 22), (8, 1500, 23), (6, 700, 24), (9, 2500, 25), (5, 400, 26), (10, 3000, 27), (7, 1000, 28)]
    ms = [synth_temporal.make_map(nk, nl, seed=s, dangling=False) for nk, nl, s in specs]
    a, b, c = ([_device_map_of(ctx, m) for m in ms] for _ in range(3))
    K = np.stack([m["K4"] for m in ms])
    before = [DM.canonical_state(x.download()) for x in a]

    L = ctx.lib
    assert L.ov2_map_triangulate_temporal_batch(ctx.h, 0, None, None, None, 1, 3.0, None) == 0
    with pytest.raises(Exception):   # a map twice
        DM.triangulate_temporal_batch(ctx, [a[0], a[0]], calib_l=K[:2])
    with pytest.raises(Exception):   # no intrinsics
        DM.triangulate_temporal_batch(ctx, a, calib_l=None)
    with pytest.raises(Exception):   # a keyframe the map does not hold
        DM.triangulate_temporal_batch(ctx, a, newkf=[m["n_kf"] + 3 for m in ms], calib_l=K)
    with pytest.raises(Exception):
        DM.triangulate_temporal_batch(ctx, a, newkf=[-1] * 8, calib_l=K)
    assert [DM.canonical_state(x.download()) for x in a] == before

    outs = DM.triangulate_temporal_batch(ctx, a, calib_l=K, stereo=True, max_reproj_err=TR.MAX_REPROJ_ERR)
    DM.triangulate_temporal_batch(ctx, c, calib_l=K, stereo=True, max_reproj_err=TR.MAX_REPROJ_ERR, want_lists=False)
    for k, (ma, mb, mc, o) in enumerate(zip(a, b, c, outs)):
        o1 = mb.triangulate_temporal_batch(calib_l=K[k], stereo=True, max_reproj_err=TR.MAX_REPROJ_ERR)[0]
        assert o["selected"] == o1["selected"] and o["candidates"] == o1["candidates"] and len(o["good_lmid"]) > 5
        for key in ("good_lmid", "good_wpt", "good_invdepth", "removed_lmid"):
            assert np.array_equal(o[key], o1[key]), (k, key)
        da, db, dc = _tables(ma), _tables(mb), _tables(mc)
        for key in da:
            assert np.array_equal(da[key], db[key]) and np.array_equal(da[key], dc[key]), (k, key)
        assert DM.canonical_state(da) != before[k]
    # a second call finds nothing left to triangulate among the landmarks it turned 3D, and removes nothing twice
    again = DM.triangulate_temporal_batch(ctx, a, calib_l=K, stereo=True, max_reproj_err=TR.MAX_REPROJ_ERR)
    for o, o2 in zip(outs, again):
        assert o2["selected"] == o["selected"] - len(o["good_lmid"]) - len(o["removed_lmid"])
        assert len(o2["good_lmid"]) == 0 and len(o2["removed_lmid"]) == 0
    for x in a + b + c:
        x.close()


def _with_2d_landmarks(ctx, P, n2d, seed):
    """the map of a local-BA window (every landmark 3D) + n2d landmarks that nobody triangulated yet, seen by the newest
    keyframe and two older ones (pixels with 0.3 px noise, every tenth a mismatch)"""
    rng = np.random.default_rng(seed)
    nk, nl = len(P.pose), len(P.lm)
    kf_all, _, _, _, _ = DM.observations_of(P)
    dm = DM.DeviceMap.from_problem(ctx, P, isobs="newest", spare=(8, n2d + 8, 3 * n2d + 64))
    Kc = P.calib_l
    Rn, tn = synth_ba.quat_to_rot(P.pose[nk - 1, 3:]), P.pose[nk - 1, :3]
    pc = np.stack([rng.uniform(-1.5, 1.5, n2d), rng.uniform(-1.0, 1.0, n2d), rng.uniform(3.0, 8.0, n2d)], 1)
    X = pc @ Rn.T + tn
    ids = np.arange(nl, nl + n2d, dtype=np.int32)
    dm.set_landmarks(ids, np.zeros((n2d, 3)), np.full(n2d, DM.LM_ALIVE | DM.LM_OBS, np.uint8))
    rows = 0
    for k in (nk - 4, nk - 2, nk - 1):
        R, t = synth_ba.quat_to_rot(P.pose[k, 3:]), P.pose[k, :3]
        q = (X - t) @ R
        uv = np.stack([Kc[0] * q[:, 0] / q[:, 2] + Kc[2], Kc[1] * q[:, 1] / q[:, 2] + Kc[3]], 1) + rng.normal(0, 0.3, (n2d, 2))
        if k == nk - 1:
            uv[::10] += rng.uniform(6, 40, (len(uv[::10]), 2))
        ok = (q[:, 2] > 0.5) & (uv[:, 0] > 0) & (uv[:, 0] < 752) & (uv[:, 1] > 0) & (uv[:, 1] < 480)
        dm.add_keyframe(k, P.pose[k], ids[ok], uv[ok].astype(np.float32).astype(np.float64))
        rows += int(ok.sum())
    assert rows > 2 * n2d
    return dm, ids


def _solve_on_device(ctx, maps, views, proto):
    pcs, rcs = DM.problems_of(views, proto, True)
    o = local_ba.default_options()
    st = ctx.lib.ov2_ba_solve_batch_dev(ctx.h, len(maps), pcs, C.byref(o), rcs)
    assert st == 0, ctx.lib.ov2_last_error(ctx.h)
    return rcs


def test_between_setup_and_update(ctx):
    """set-up -> temporal call -> solve -> update: the update is accepted and ends where the same sequence ends with the
    temporal call's edits applied by hand through ov2_map_set_landmarks + ov2_map_remove_obs"""
    P = synth_ba.make_window(12, 900, inv_depth=True, seed=77, outlier_frac=0.08)
    P.res_uv = P.res_uv.astype(np.float32).astype(np.float64)
    P.lm_anchor_uv = P.lm_anchor_uv.astype(np.float32).astype(np.float64)
    (a, ids), (b, _) = _with_2d_landmarks(ctx, P, 400, 5), _with_2d_landmarks(ctx, P, 400, 5)
    assert DM.canonical_state(a.download()) == DM.canonical_state(b.download())
    va, vb = DM.setup_batch(ctx, [a], calib_l=P.calib_l), DM.setup_batch(ctx, [b], calib_l=P.calib_l)
    assert not va[0].aborted and va[0].n_res == vb[0].n_res > 1000
    flat = DM.fetch_view(ctx, va[0], True)
    assert not np.isin(ids, flat["lm_lmid"]).any()

    out = a.triangulate_temporal_batch(calib_l=P.calib_l, stereo=True, max_reproj_err=3.0)[0]
    assert len(out["good_lmid"]) > 100 and len(out["removed_lmid"]) > 5, (len(out["good_lmid"]), len(out["removed_lmid"]))
    st_b = b.download()["lm_state"]
    b.set_landmarks(out["good_lmid"], out["good_wpt"], (st_b[out["good_lmid"]] | DM.LM_3D | DM.LM_KP3D).astype(np.uint8))
    b.remove_obs(np.full(len(out["removed_lmid"]), b.newkf, np.int32), out["removed_lmid"])
    assert DM.canonical_state(a.download()) == DM.canonical_state(b.download())

    ra, rb = _solve_on_device(ctx, [a], va, P), _solve_on_device(ctx, [b], vb, P)
    assert ra[0].n_outliers_pass1 == rb[0].n_outliers_pass1 > 0
    ua = DM.update_batch(ctx, [a], va, cur_kfid=[a.newkf])[0]     # accepted: the temporal call did not end the set-up
    ub = DM.update_batch(ctx, [b], vb, cur_kfid=[b.newkf])[0]
    assert np.array_equal(ua["removed_lmid"], ub["removed_lmid"]) and len(ua["removed_obs"]) == len(ub["removed_obs"]) > 0
    assert {tuple(x) for x in ua["removed_obs"]} == {tuple(x) for x in ub["removed_obs"]}
    assert {tuple(x) for x in ua["stereo_off"]} == {tuple(x) for x in ub["stereo_off"]}
    da, db = _tables(a), _tables(b)
    for key in da:
        assert np.array_equal(da[key], db[key]), key
    # the landmarks the temporal call turned 3D are outside this window: the update left them where the call put them
    assert np.array_equal(da["lm_xyz"][out["good_lmid"]], out["good_wpt"])
    a.close(); b.close()


def _loop(ctx, scene, n, temporal):
    cl = host_map.CppSlam(ctx, synth_scene.K4, synth_scene.BASELINE, synth_scene.W, synth_scene.H, policy="slam_loop", kf_every=5,
                          ba_window=0, device_map=True)
    if temporal is not None:
        cl.set_temporal(temporal)
    try:
        for t in range(n):
            ir = scene.right(t).copy()
            ir[:, 300:460] = 128          # the stereo matcher never finds the stripe's keypoints in the right image
            cl.step(0.05 * t, scene.left(t), ir)
        inv, total = cl.check_map()
        host = cl.export_map()
        cl.flush_device()
        raw = DM.DeviceMap.download(_Handle(ctx, cl.device_handle()))
    finally:
        cl.close()
    return cl, inv, total, host, raw


def _stripe(host, raw, kf):
    """landmarks keyframe kf observes whose keypoint stood inside the band in every keyframe that saw them (left pixel in
    [325, 450]: with 8 to 12 px of disparity and the tracker's 9 px window, all of its right-image window is grey) and that
    no keyframe matched in the right image"""
    _, lm_h, ob_h = host
    live = (raw["obs_flag"] & DM.OBS_ALIVE).astype(bool)
    x = raw["obs_uv"][:, 0]
    outside = set(raw["obs_lm"][live & ((x < 325) | (x > 450))].tolist())
    stereo = {l for (k, l), s in ob_h.items() if s}
    return sorted(l for (k, l) in ob_h if k == kf and l in lm_h and l not in outside and l not in stereo)


def test_closed_loop_recovers_the_stripe(ctx):
    """a grey band over columns 300-460 of every RIGHT image: the keypoints of that stripe never get a stereo match.  Without
    the stage (the default, and the behaviour before it existed) their landmarks stay 2D for good; with it they turn 3D as
    soon as two keyframes see them, they lie on the plane, the host map keeps its invariants, the mirror follows, and the
    trajectory stays on the ground truth."""
    n = 40
    scene = synth_scene.PlaneScene(n)
    gt = [scene.pose(t) for t in range(n)]
    off, inv_off, _, host_off, raw_off = _loop(ctx, scene, n, None)
    stripe_off = _stripe(host_off, raw_off, max(host_off[0]))
    print(f"[temporal loop] off: {len(stripe_off)} stripe landmarks in the last keyframe, "
          f"{sum(bool(host_off[1][l][1] & 2) for l in stripe_off)} of them 3D; invariants {inv_off}")
    assert len(stripe_off) >= 10 and not any(host_off[1][l][1] & 2 for l in stripe_off), "the stripe is 3D without the stage?"
    assert slam_loop.ate_rmse(off.traj, gt) < 0.01

    on, inv, total, host, raw = _loop(ctx, scene, n, True)
    dev = DM.canonical_state(raw)
    ts = on.temporal_stats
    stripe = _stripe(host, raw, max(host[0]))
    rec = [l for l in stripe if host[1][l][1] & 2]
    print(f"[temporal loop] stripe landmarks in the last keyframe: {len(stripe_off)} (off, all 2D) / {len(stripe)} (on), "
          f"{len(rec)} of them 3D = {len(rec) / max(len(stripe), 1):.2f}; per keyframe {ts}")
    assert len(ts) == 8 and ts[0]["ran"] == 0 and all(t["ran"] for t in ts[2:])
    assert len(rec) >= 10, ts
    xyz = np.array([host[1][l][0] for l in rec])
    dist = np.abs(xyz @ scene.nrm - scene.d)
    print(f"[temporal loop] median |xyz.n - d| of the recovered landmarks = {np.median(dist):.4f} m, ATE = "
          f"{slam_loop.ate_rmse(on.traj, gt):.5f} m")
    assert np.median(dist) < 0.05
    assert total == 0, inv
    assert slam_loop.ate_rmse(on.traj, gt) < 0.01
    kf_h, lm_h, ob_h = host
    kf_d, lm_d, ob_d = dev
    assert sorted(kf_h) == sorted(kf_d) and all(np.allclose(kf_h[k], kf_d[k], atol=1e-12) for k in kf_h)
    assert sorted(lm_h) == sorted(lm_d)
    assert set(ob_h) == set(ob_d)
    assert all(bool(ob_h[o]) == bool(ob_d[o]) for o in ob_h)
    # points and 3D flags too: what the stage wrote reached the mirror
    assert all((lm_h[l][1] & 2) == (lm_d[l][1] & 2) for l in lm_h)
    assert all(np.allclose(lm_h[l][0], lm_d[l][0], atol=1e-12) for l in lm_h if lm_h[l][1] & 2)
