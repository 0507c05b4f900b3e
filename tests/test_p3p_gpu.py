"""GPU tests of the P3P stage of computePose (ov2_p3p_ransac_batch, csrc/p3p.hip) against the numpy restatement
tests/p3p_ref.py, whose P3P solver is another method (Grunert's quartic + Procrustes) than the kernel's (Kneip).
Bar: integer outcomes (status, info, outlier mask) identical, Twc within 1e-8 (the bar of the epipolar stage)."""
import numpy as np
import pytest

import p3p_ref as PR
from ov2slam_amd import synth_p3p
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

pytestmark = pytest.mark.gpu
ERRTH = 3.0
GAP = 1e-6      # a scene takes part in the exact comparison only if the checker's smallest relative gaps exceed this


def _one(mvg, s, nmaxiter, seed, lmeds=True, T0=None):
    r = mvg.p3pRansac_batch([s["bv"]], [s["wpts"]], nmaxiter, ERRTH, s["K"][None], [seed], lmeds, T0)
    return {k: v[0] for k, v in r.items()}


def _same_pose(Tg, Te, tol=1e-8):
    q = Tg[3:] if np.dot(Tg[3:], Te[3:]) >= 0 else -Tg[3:]
    return np.abs(Tg[:3] - Te[:3]).max() < tol and np.abs(q - Te[3:]).max() < tol


# ---- 1. device solver ---------------------------------------------------------------------------------------------------
def test_device_solver(ctx):
    """ov2_dbg_p3p on 5000 exact samples of the scene generator.  Every device solution is a rotation that maps the three
    points onto their bearings with positive depth; the ground truth is among the solutions and the set equals numpy's
    (Grunert) except on counted samples, which stay below 0.1 % of the samples."""
    bv, X, Rg, tg = synth_p3p.random_samples(5000, seed=13)
    R, t, ns = MultiViewGeometry(ctx).dbg_p3p(bv, X)
    exceptions = 0
    for i in range(len(ns)):
        assert 0 <= ns[i] <= 4
        for s in range(ns[i]):
            r = R[i, s]
            assert np.abs(r @ r.T - np.eye(3)).max() < 1e-9 and np.linalg.det(r) > 0
            p = (X[i] - t[i, s]) @ r
            assert ((p * bv[i]).sum(1) > 0).all()
            assert np.abs(p / np.linalg.norm(p, axis=1, keepdims=True) - bv[i]).max() < 1e-9
        has_gt = any(np.abs(R[i, s] - Rg[i]).max() < 1e-7 and np.abs(t[i, s] - tg[i]).max() < 1e-7 for s in range(ns[i]))
        S = PR.p3p_grunert(bv[i], X[i])
        same = len(S) == ns[i] and all(any(np.abs(R[i, s] - r).max() < 1e-6 and np.abs(t[i, s] - tt).max() < 1e-6
                                           for s in range(ns[i])) for r, tt in S)
        exceptions += not (has_gt and same)
    print(f"solver exceptions: {exceptions} of {len(ns)}; solutions per sample {np.bincount(ns, minlength=5).tolist()}")
    assert exceptions < 0.001 * len(ns)


# ---- 2. single frame against the restatement -----------------------------------------------------------------------------
def _qualifying_scene(n, frac, nmaxiter, lmeds, seed):
    """the scene of the case and the checker's result; for n >= 30 the seed is changed until both gaps exceed GAP"""
    for k in range(8):
        s = synth_p3p.make_scene(n, seed=1000 * k + n + int(frac * 100) + nmaxiter, outlier_frac=frac, noise_px=0.3)
        e = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], nmaxiter, ERRTH, lmeds, seed)
        if n < 30 or (e["gaps"]["penalty"] > GAP and e["gaps"]["score"] > GAP):
            return s, e
    raise AssertionError("no qualifying scene")


@pytest.mark.parametrize("n", [4, 5, 6, 9, 30, 308, 2048, 4096])
@pytest.mark.parametrize("frac", [0.0, 0.2, 0.4])
@pytest.mark.parametrize("nmaxiter", [1, 100])
@pytest.mark.parametrize("lmeds", [True, False], ids=["lmeds", "ransac"])
def test_single_frame_matches_restatement(ctx, n, frac, nmaxiter, lmeds):
    seed = 99 + n
    s, e = _qualifying_scene(n, frac, nmaxiter, lmeds, seed)
    g = _one(MultiViewGeometry(ctx), s, nmaxiter, seed, lmeds)
    print(f"n {n} frac {frac} it {nmaxiter} lmeds {lmeds}: gpu status {g['status']} info {list(g['info'])} | ref status "
          f"{e['status']} info {e['info']} gaps {e['gaps']['penalty']:.3g} {e['gaps']['score']:.3g}")
    exact = n >= 30 or (e["gaps"]["penalty"] > GAP and e["gaps"]["score"] > GAP)
    if exact or not lmeds:
        assert g["status"] == e["status"] and list(g["info"]) == e["info"]
        assert np.array_equal(g["outlier"], e["outlier"])
        if e["status"] == 1:
            assert _same_pose(g["Twc"], e["Twc"])
        return
    # n < 30 with a near-tie.  The counts of counted / skipped draws stay exact.
    assert list(g["info"][:2]) == e["info"][:2]
    dg, de = int(g["info"][2]), e["info"][2]
    assert (dg < 0) == (de < 0)
    if n >= 6:
        # A near-tie is the same three points in another order (or with another fourth): the same model to rounding.  The
        # kernel's draw must be one of the checker's draws tied with its winner, and status, inlier count, outlier mask and
        # pose (1e-8) must be the checker's result under THAT draw's model.  Tied = within GAP relative; for n = 6 only, plus
        # 2e-8: there the penalty is (sqrt(d[2]) + sqrt(d[3])) / 2 and d[2] is the sample's own third residual, 0 to a few
        # quanta q = 1.11e-16 of 1 - cos (measured on these scenes: re-ordered triples differ by exactly sqrt(q) / 2 =
        # 5.27e-9); sqrt(4 q) / 2 = 1.05e-8 per draw, two draws.  From n = 7 on the median is free of sample residuals.
        if dg >= 0:
            tied = PR.tied_results(s["bv"], s["wpts"], e, GAP, 2e-8 if n == 6 else 0.)
            assert dg in tied, (dg, sorted(tied))
            assert sorted(PR.draw(seed, dg, n)[:3]) == sorted(PR.draw(seed, de, n)[:3])      # the checker's triple
            st, Twc, out, ninl = tied[dg]
            assert g["status"] == st and g["info"][3] == ninl and np.array_equal(g["outlier"], out)
            if st == 1:
                assert _same_pose(g["Twc"], Twc)
        else:
            assert g["status"] == 0 and not g["outlier"].any()
        return
    # n = 4, 5: the median itself is one of the sample's own residuals, i.e. rounding noise (sqrt of the 1.1e-16 quantum of
    # 1 - cos: 1e-8), so which draw wins is not defined beyond "terminates with a well-defined status": the status follows
    # the rule, and if the kernel chose the checker's sample everything is compared.
    assert g["status"] == int(dg >= 0 and g["info"][3] >= 5)
    if dg >= 0:
        ig, ie = PR.draw(seed, dg, n), PR.draw(seed, de, n)
        if sorted(ig[:3]) == sorted(ie[:3]) and ig[3] == ie[3]:
            assert g["status"] == e["status"] and g["info"][3] == e["info"][3]
            assert np.array_equal(g["outlier"], e["outlier"])
            if e["status"] == 1:
                assert _same_pose(g["Twc"], e["Twc"])


# ---- 3. ground truth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [30, 308, 2048, 4096])
@pytest.mark.parametrize("frac", [0.0, 0.2, 0.4])
def test_single_frame_ground_truth(ctx, n, frac):
    """noise-free scenes, 100 draws, LMedS: the injected outliers and nothing else are flagged, the pose is within 1e-6 of
    the truth (1 - cos is quantised at 1.1e-16, so models within about 1.5e-8 rad share a penalty: 4e-7 m at 25 m)"""
    s = synth_p3p.make_scene(n, seed=n + int(frac * 100) + 100, outlier_frac=frac, noise_px=0.0)
    g = _one(MultiViewGeometry(ctx), s, 100, 99 + n)
    assert g["status"] == 1 and g["info"][0] == 100
    assert np.array_equal(g["outlier"], s["outlier"])
    assert _same_pose(g["Twc"], s["Twc"], 1e-6)


# ---- 4. batch and forms -----------------------------------------------------------------------------------------------------
def _batch_inputs(B=64):
    rng = np.random.default_rng(4)
    sizes = rng.choice([4, 5, 9, 30, 64, 200, 308, 700, 1500, 2048], B)
    sizes[:6] = [0, 3, 4, 308, 2048, 4500]
    scenes = [synth_p3p.make_scene(int(k), seed=1000 + b, outlier_frac=[0., 0.2, 0.4, 0.9][b % 4]) for b, k in enumerate(sizes)]
    K = np.array([s["K"] for s in scenes])
    seeds = [3 * b + 1 for b in range(B)]
    return scenes, K, seeds


@pytest.mark.parametrize("lmeds", [True, False], ids=["lmeds", "ransac"])
def test_batch_equals_single_calls(ctx, lmeds):
    mvg = MultiViewGeometry(ctx)
    scenes, K, seeds = _batch_inputs()
    B = len(scenes)
    T0 = np.tile([7., -3., 2., 0.5, 0.5, 0.5, 0.5], (B, 1))
    r = mvg.p3pRansac_batch([s["bv"] for s in scenes], [s["wpts"] for s in scenes], 100, ERRTH, K, seeds, lmeds, T0)
    assert list(r["status"][:2]) == [0, 0] and list(r["info"][0]) == [0, 0, -1, 0] and list(r["info"][1]) == [0, 0, -1, 0]
    assert set(r["status"].tolist()) == {0, 1}
    for b, s in enumerate(scenes):
        q = mvg.p3pRansac_batch([s["bv"]], [s["wpts"]], 100, ERRTH, K[b:b + 1], [seeds[b]], lmeds, T0[b:b + 1])
        assert r["status"][b] == q["status"][0] and np.array_equal(r["info"][b], q["info"][0])
        assert r["Twc"][b].tobytes() == q["Twc"][0].tobytes()
        assert np.array_equal(r["outlier"][b], q["outlier"][0])
        if r["status"][b] == 0:
            assert r["Twc"][b].tobytes() == T0[b].tobytes() and not r["outlier"][b].any()


@pytest.mark.parametrize("lmeds", [True, False], ids=["lmeds", "ransac"])
def test_dev_form_equals_host_form(ctx, lmeds):
    mvg = MultiViewGeometry(ctx)
    scenes, K, seeds = _batch_inputs(16)
    B = len(scenes)
    T0 = np.tile([7., -3., 2., 0.5, 0.5, 0.5, 0.5], (B, 1))
    host = mvg.p3pRansac_batch([s["bv"] for s in scenes], [s["wpts"] for s in scenes], 100, ERRTH, K, seeds, lmeds, T0)
    off = np.concatenate([[0], np.cumsum([len(s["bv"]) for s in scenes])]).astype(np.int32)
    d = ctx.to_device
    d_out, d_T = ctx.empty(max(off[-1], 1), np.uint8), d(T0)
    d_st, d_in = ctx.empty(B, np.int32), ctx.empty((B, 4), np.int32)
    mvg.p3pRansac_batch_dev(B, d(off), d(np.concatenate([s["bv"] for s in scenes])), d(np.concatenate([s["wpts"] for s in scenes])),
                            d(K), 100, ERRTH, lmeds, d(np.array(seeds, np.uint64)), d_T, d_out, d_st, d_in)
    ctx.synchronize()
    assert np.array_equal(d_st.get(), host["status"]) and np.array_equal(d_in.get(), host["info"])
    assert np.array_equal(d_out.get()[:off[-1]].astype(bool), np.concatenate(host["outlier"]))
    assert d_T.get().tobytes() == host["Twc"].tobytes()


@pytest.mark.parametrize("lmeds,frac,seed,block", [(True, 0.2, 26, 0), (True, 0.2, 13, 1), (False, 0.85, 12, 0)],
                         ids=["lmeds-winner-in-block-0", "lmeds-winner-in-block-1", "ransac-3001-iterations"])
def test_more_draws_than_one_block(ctx, lmeds, frac, seed, block):
    """nmaxiter = 3000: the first chain of launches covers 2 * 256 + 32 = 544 draws, the following ones 2817 each, so the
    loop's state (counts, the best so far and its 'strictly lower' rule, RANSAC's bound k) is carried from block to block.
    LMedS: the checker's winner is draw 95 (first block) for one seed and draw 3007 (a later block) for the other; RANSAC at
    85 % outliers runs all 3001 iterations.  Everything is compared, the chosen draw included (the scenes' penalty gaps are
    1e-3 and more)."""
    s = synth_p3p.make_scene(100, seed=77 if lmeds else 78, outlier_frac=frac, noise_px=0.3)
    g = _one(MultiViewGeometry(ctx), s, 3000, seed, lmeds)
    e = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], 3000, ERRTH, lmeds, seed)
    assert e["info"][0] + e["info"][1] > 544 and (e["info"][2] >= 544) == bool(block)
    assert not lmeds or e["gaps"]["penalty"] > GAP
    assert g["status"] == e["status"] == 1 and list(g["info"]) == e["info"]
    assert np.array_equal(g["outlier"], e["outlier"]) and _same_pose(g["Twc"], e["Twc"])


# ---- 5. edges that must end with a defined status ------------------------------------------------------------------------
def test_too_few_points(ctx):
    mvg = MultiViewGeometry(ctx)
    T0 = np.array([[1., 2., 3., 0., 0., 0., 1.]])
    for n in (0, 1, 3):
        s = synth_p3p.make_scene(n, seed=3, outlier_frac=0.0)
        for lmeds in (True, False):
            g = _one(mvg, s, 100, 1, lmeds, T0)
            assert g["status"] == 0 and list(g["info"]) == [0, 0, -1, 0] and not g["outlier"].any()
            assert g["Twc"].tobytes() == T0[0].tobytes()


@pytest.mark.parametrize("kind", ["identical", "collinear", "zero_bearing", "nan", "mostly_nan", "all_outliers", "no_draws"])
def test_degenerate_inputs_terminate(ctx, kind):
    rng = np.random.default_rng(17)
    s = synth_p3p.make_scene(200, seed=30, outlier_frac=0.1)
    nmaxiter = 50
    if kind == "identical":
        s["wpts"][:] = s["wpts"][0]
        s["bv"][:] = s["bv"][0]
    elif kind == "collinear":
        s["wpts"] = s["wpts"][0] + np.outer(rng.uniform(-5, 5, 200), [1., 2., 0.5])
    elif kind == "zero_bearing":
        s["bv"][::7] = 0.
    elif kind == "nan":
        s["bv"][5] = np.nan
        s["wpts"][11, 1] = np.nan
    elif kind == "mostly_nan":      # 60 % spoiled: 97 % of the draws have no model, the loop runs into its skip budget
        s["bv"][:120] = np.nan          # in the block behind the first one with a few counted draws
    elif kind == "all_outliers":
        s["bv"] = s["bv"][rng.permutation(200)]
    elif kind == "no_draws":
        nmaxiter = 0
    for lmeds in (True, False):
        g = _one(MultiViewGeometry(ctx), s, nmaxiter, 9, lmeds)
        e = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], nmaxiter, ERRTH, lmeds, 9)
        assert g["info"][0] + g["info"][1] <= 11 * nmaxiter + 1
        assert g["status"] == e["status"]
        if kind == "zero_bearing":
            # a zero bearing as the 4th point scores 1 under every candidate: an exact tie that the two solvers break by
            # their root orders, so the chosen draws may differ; the pose must still be the scene's, the spoiled ones out
            assert g["status"] == 1 and _same_pose(g["Twc"], s["Twc"], 0.05) and g["outlier"][::7].all()
            continue
        assert list(g["info"]) == e["info"] and np.array_equal(g["outlier"], e["outlier"])
        if kind in ("identical", "collinear", "no_draws"):
            assert g["status"] == 0 and g["info"][2] == -1
        if kind == "mostly_nan":
            assert g["info"][1] == 10 * nmaxiter and 0 < g["info"][0] < nmaxiter and g["outlier"][:120].all() == (g["status"] == 1)
        if kind == "nan":      # the spoiled correspondences are never inliers, the rest still gives the pose
            assert g["status"] == 1 and _same_pose(g["Twc"], e["Twc"]) and g["outlier"][[5, 11]].all()


def test_argument_checks(ctx):
    mvg = MultiViewGeometry(ctx)
    s = synth_p3p.make_scene(50, seed=2)
    with pytest.raises(Exception, match="nmaxiter"):
        mvg.p3pRansac_batch([s["bv"]], [s["wpts"]], (1 << 20) + 1, ERRTH, s["K"][None], [1])
    with pytest.raises(Exception, match="nmaxiter"):
        mvg.p3pRansac_batch([s["bv"]], [s["wpts"]], -1, ERRTH, s["K"][None], [1])
    with pytest.raises(Exception, match="above 65535"):      # OV2_P3P_MAX_BATCH: an argument error, not a launch error
        mvg.p3pRansac_batch([np.zeros((0, 3))] * 65536, [np.zeros((0, 3))] * 65536, 100, ERRTH, np.tile(s["K"], (65536, 1)),
                            np.arange(65536))
    with pytest.raises(NotImplementedError):
        mvg.p3pRansac(s["bv"], s["wpts"], 100, ERRTH, True, True, 458., 458.)
    with pytest.raises(ValueError):
        mvg.p3pRansac_batch([s["bv"]], [s["wpts"][:-1]], 100, ERRTH, s["K"][None], [1])
    r = mvg.p3pRansac_batch([], [], 100, ERRTH, np.zeros((0, 4)), [])
    assert len(r["status"]) == 0
    ok, T, idx = mvg.p3pRansac(s["bv"], s["wpts"], 100, ERRTH, False, True, 458., 458., seed=4)
    e = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], 100, ERRTH, True, 4)
    assert ok and idx.tolist() == np.flatnonzero(e["outlier"]).tolist() and _same_pose(T, e["Twc"])


# ---- 6. the host stage: VisualFrontEnd::computePose with its P3P branch ---------------------------------------------------
def _pose_frame(scene):
    """a host map with one keyframe observing the scene's landmarks (ids = indices), its pose to be set by compute_pose"""
    from ov2slam_amd import host_map
    f = host_map.FrontEndFrame(scene["K"], 0.11, synth_p3p.W, synth_p3p.H)
    kps = {}
    for i, (px, X) in enumerate(zip(scene["px"], scene["wpts"])):
        f.add_keypoint(i, px, X)
        kps[i] = (np.asarray(px, np.float32), X)
    return f, kps


def _off_pose(scene, dt, deg):
    """the scene's pose moved by dt metres and turned by deg degrees"""
    from ov2slam_amd import synth_ba
    dR, _ = synth_ba.se3_exp(np.array([0, 0, 0, 0, np.deg2rad(deg), 0]))
    return synth_ba.pose7(dR @ scene["R"], scene["t"] + np.array([dt, 0, 0]))


def _near_truth(T, scene):
    """translation within 2e-2 m (the bar of the ceresPnP tests against the truth), quaternion within 5e-3"""
    q = T[3:] if np.dot(T[3:], scene["Twc"][3:]) >= 0 else -T[3:]
    return np.abs(T[:3] - scene["Twc"][:3]).max() < 2e-2 and np.abs(q - scene["Twc"][3:]).max() < 5e-3


def test_host_stage_dop3p(ctx, oracle):
    """(a) dop3p_ set: computePose from a pose 1 m / 20 deg off recovers the pose through P3P + ceresPnP, removes the displaced
    observations and no others, and equals the transcription of the reference function driven by the checker"""
    s = synth_p3p.make_scene(320, seed=601, outlier_frac=0.2, noise_px=0.3)
    f, kps = _pose_frame(s)
    try:
        f.set_p3p(True, 100, ERRTH, False, seed=17)
        T0 = _off_pose(s, 1.0, 20.)
        st, req = f.compute_pose(ctx, T0)
        assert st == 0 and not req            # OV2_ERR_UNSUPPORTED before the stage existed
        e = PR.compute_pose(oracle.pnp_solve, kps, s["K"], T0, False, True, False, 100, ERRTH, 17)
        left = sorted(f.keypoints())
        removed = [i for i in range(320) if i not in left]
        assert removed == e["removed"] == np.flatnonzero(s["outlier"]).tolist()
        ps = f.p3p_stats()
        assert ps == dict(ran=1, status=1, points=320, removed=int(e["p3p"]["outlier"].sum()), reset=0)
        assert _near_truth(f.pose(), s) and _same_pose(f.pose(), e["Twc"], 1e-7)
        assert all(f.landmark_isobs(i) == 0 for i in removed) and f.counters()["nb3dkps"] == 320 - len(removed)
    finally:
        f.close()


def test_host_stage_p3p_request(ctx, oracle):
    """(b) dop3p_ off: a start pose so far off that ceresPnP is rejected sets bp3preq_ and leaves the frame alone; the next
    call from the same pose runs the P3P branch and succeeds"""
    s = synth_p3p.make_scene(320, seed=602, outlier_frac=0.2, noise_px=0.3)
    f, kps = _pose_frame(s)
    try:
        f.set_p3p(False, 100, ERRTH, False, seed=23)
        T0 = e1 = None
        for dt, deg in [(1.0, 20.), (2.0, 40.), (4.0, 80.), (8.0, 150.)]:      # the first one the oracle's PnP rejects
            T0 = _off_pose(s, dt, deg)
            e1 = PR.compute_pose(oracle.pnp_solve, kps, s["K"], T0, False, False, False, 100, ERRTH, 23)
            if e1["p3p_req"]:
                break
        assert e1["p3p_req"] and not e1["removed"]
        st, req = f.compute_pose(ctx, T0)
        assert st == 0 and req and f.p3p_stats()["ran"] == 0
        assert len(f.keypoints()) == 320 and f.pose().tobytes() == np.asarray(T0).tobytes()
        st, req = f.compute_pose(ctx, T0)
        assert st == 0 and not req
        e2 = PR.compute_pose(oracle.pnp_solve, kps, s["K"], T0, True, False, False, 100, ERRTH, 23)
        removed = [i for i in range(320) if i not in f.keypoints()]
        assert removed == e2["removed"] == np.flatnonzero(s["outlier"]).tolist()
        assert f.p3p_stats()["ran"] == 1 and f.p3p_stats()["status"] == 1 and f.p3p_stats()["reset"] == 0
        assert _near_truth(f.pose(), s) and _same_pose(f.pose(), e2["Twc"], 1e-7)
    finally:
        f.close()


def test_host_stage_reset_frame(ctx, oracle):
    """(c) 80 % displaced observations: P3P finds no pose worth keeping -> resetFrame(): counters and grid zero, mapkps_
    empty, every observation withdrawn on the map side, the pose unchanged.  The generator's displacements of 8-60 px do not
    get there: on nine such scenes the checker's LMedS still ended with 7 to 64 inliers (status 1), because mildly displaced
    points keep pulling the median towards the true pose.  So the displaced 80 % of this case are moved anywhere in the
    image; the checker then ends with 3 or 4 inliers on five scenes of six, this being the first."""
    s = synth_p3p.make_scene(320, seed=604, outlier_frac=0.8, noise_px=0.3)
    rng = np.random.default_rng(604)
    bad = np.flatnonzero(s["outlier"])
    s["px"][bad] = np.stack([rng.uniform(20, 732, len(bad)), rng.uniform(20, 460, len(bad))], 1)
    f, kps = _pose_frame(s)
    try:
        f.set_p3p(True, 100, ERRTH, False, seed=29)
        T0 = _off_pose(s, 1.0, 20.)
        e = PR.compute_pose(oracle.pnp_solve, kps, s["K"], T0, False, True, False, 100, ERRTH, 29)
        assert e["reset"] and e["removed"] == list(range(320))
        st, req = f.compute_pose(ctx, T0)
        assert st == 0 and not req
        ps = f.p3p_stats()
        assert ps["ran"] == 1 and ps["reset"] == 1 and ps["points"] == 320
        assert f.counters() == dict(nbkps=0, nb2dkps=0, nb3dkps=0, nb_stereo_kps=0, noccupcells=0)
        assert f.keypoints() == {} and all(f.landmark_isobs(i) == 0 for i in range(320))
        assert f.pose().tobytes() == np.asarray(T0).tobytes()
    finally:
        f.close()


def test_p3p_ransac_forms(ctx):
    """MultiViewGeometry::p3pRansac with the reference's arguments, Python and C++, against the restatement"""
    from ov2slam_amd import host_map
    mvg = MultiViewGeometry(ctx)
    T0 = np.array([1., 2., 3., 0., 0., 0., 1.])
    for n, frac, seed, lmeds in [(300, 0.2, 3, True), (40, 0.3, 4, True), (3, 0.0, 5, True), (300, 0.2, 6, False)]:
        s = synth_p3p.make_scene(n, seed=70 + seed, outlier_frac=frac)
        e = PR.p3p_ransac(s["bv"], s["wpts"], s["K"], 100, ERRTH, lmeds, seed)
        ok, T, idx = mvg.p3pRansac(s["bv"], s["wpts"], 100, ERRTH, False, True, 458., 458., T0, lmeds, seed)
        ok2, T2, idx2 = host_map.p3p_ransac(ctx, s["bv"], s["wpts"], 100, ERRTH, False, True, 458., 458., T0, lmeds, seed)
        assert ok == ok2 == (e["status"] == 1) and T.tobytes() == T2.tobytes()
        if ok:
            assert idx.tolist() == idx2.tolist() == np.flatnonzero(e["outlier"]).tolist() and _same_pose(T, e["Twc"])
        else:
            assert T.tobytes() == T0.tobytes() and len(idx) == len(idx2) == 0
    with pytest.raises(RuntimeError):
        host_map.p3p_ransac(ctx, s["bv"], s["wpts"], 100, ERRTH, True, True, 458., 458., T0)


# ---- 7. frame loop --------------------------------------------------------------------------------------------------------
def _p3p_loop(ctx, scene, frames, dop3p, seed=5):
    from ov2slam_amd import host_map, synth_scene
    cl = host_map.CppSlam(ctx, synth_scene.K4, synth_scene.BASELINE, synth_scene.W, synth_scene.H, policy=None, device_map=True)
    try:
        cl.set_epipolar(False, 100, ERRTH, True, seed)      # nransac_iter / fransac_err / bdo_random / seed of both stages
        cl.set_p3p(dop3p)
        for k, t in enumerate(frames):
            cl.step(0.05 * k, scene.left(t), scene.right(t))   # raises unless addNewStereoImages returns OV2_OK
    finally:
        cl.close()
    return cl


def test_frame_loop_with_p3p(ctx):
    """SlamManager with dop3p_ on the plane sequence of tests/test_closed_loop.py: every frame bootstraps its pose by
    P3P-LMedS before ceresPnP.  Same ATE bound as the epipolar loop test; two runs are bitwise equal."""
    from ov2slam_amd import slam_loop, synth_scene
    scene = synth_scene.PlaneScene(40)
    n = 64
    a = _p3p_loop(ctx, scene, range(n), True)
    gt = [scene.pose(t) for t in range(n)]
    assert slam_loop.ate_rmse(a.traj, gt) < 0.01
    assert a.p3p_stats[0]["ran"] == 0
    assert all(p["ran"] == 1 and p["status"] == 1 and p["reset"] == 0 for p in a.p3p_stats[1:])
    b = _p3p_loop(ctx, scene, range(n), True)
    assert np.array_equal(np.array(a.traj).view(np.uint64), np.array(b.traj).view(np.uint64))
    assert a.p3p_stats == b.p3p_stats


def test_frame_loop_kidnap(ctx):
    """dop3p_ off, and 20 frames of the stream dropped after frame 19: on the next frame fewer than 33 % of the prior-based
    tracks survive, kltTracking sets bp3preq_, and computePose recovers the pose by P3P-LMedS where the loop used to stop with
    OV2_ERR_UNSUPPORTED.  (Gaps of 6 and 10 frames do not fire the rule on that frame, 14 to 28 do; at 20 the branch sees 179
    3D tracks.)  The poses after the gap stay within the bound of the loop tests."""
    from ov2slam_amd import slam_loop, synth_scene
    scene = synth_scene.PlaneScene(40)
    start, gap = 20, 20
    frames = list(range(start)) + list(range(start + gap, start + gap + 24))
    a = _p3p_loop(ctx, scene, frames, False)
    assert len(a.traj) == len(frames)                      # no frame ended the loop
    assert not any(p["ran"] for p in a.p3p_stats[:start])  # easy frames never ask for P3P
    hit = a.p3p_stats[start]
    assert hit["ran"] == 1 and hit["points"] >= 4 and (hit["status"] == 1 or hit["reset"] == 1)
    gt = [scene.pose(t) for t in frames]
    assert slam_loop.ate_rmse(a.traj[start + 1:], gt[start + 1:]) < 0.01
    b = _p3p_loop(ctx, scene, frames, False)
    assert np.array_equal(np.array(a.traj).view(np.uint64), np.array(b.traj).view(np.uint64)) and a.p3p_stats == b.p3p_stats
