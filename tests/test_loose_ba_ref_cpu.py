"""The numpy statement of Optimizer::looseBA (tests/loose_ba_ref.py) against the host stage (Optimizer::setupRangeBA /
applyLooseBA of ov2slam_amd/host, reference src/optimizer.cpp:900-1672) -- no GPU: the range selection keyed by ids, the six
update steps on crafted states and flags, and the conditions the scenes of tests/loose_ba_cases.py must meet (landmarks
whose oldest observer is younger than the loop keyframe; chi2 margins of the whole-statement scenes)."""
import numpy as np
import pytest

from ov2slam_amd import ba_types as T
from ov2slam_amd import host_map

import loose_ba_cases as LC
import loose_ba_ref as LR

SCENES = {
    "12kf": dict(n_kf=12, n_lm=600, ini=3, n=8, seed=35),
    "70kf": dict(n_kf=70, n_lm=400, ini=5, n=60, seed=36, n_prop=40, min_younger=1),
    "removed": dict(n_kf=12, n_lm=600, ini=3, n=8, seed=35, rm_kfs=(3, 4)),   # the first two keyframes of the range are gone
    "one": dict(n_kf=12, n_lm=600, ini=8, n=8, seed=35),
    "empty": dict(n_kf=12, n_lm=600, ini=9, n=8, seed=35),
}


def canon(pb):
    poses = {int(k): (int(c), tuple(p)) for k, c, p in zip(pb["pose_kfid"], pb["pose_const"], pb["pose"])}
    lms = {int(l): (tuple(v), int(a), tuple(uv)) for l, v, a, uv in zip(pb["lm_lmid"], pb["lm"], pb["lm_anchor_kfid"], pb["lm_anchor_uv"])}
    res = sorted((int(t), int(k), int(l), float(uv[0]), float(uv[1]))
                 for t, k, l, uv in zip(pb["res_type"], pb["res_kfid"], pb["res_lmid"], pb["res_uv"]))
    return poses, lms, res


def assert_same_problem(a, b, inv_depth, exact=False):
    pa, la, ra = canon(a)
    pb_, lb, rb = canon(b)
    assert pa == pb_, "keyframes / constness / poses differ"
    assert ra == rb, "residual blocks differ"
    assert sorted(la) == sorted(lb), "landmark sets differ"
    for l in la:
        va, aa, ua = la[l]
        vb, ab, ub = lb[l]
        assert (aa, ua) == (ab, ub) if inv_depth else True, l
        if exact:
            assert va == vb, (l, va, vb)
        else:   # 1 / z: two roundings of R'(p - t)
            assert np.allclose(va, vb, rtol=1e-12, atol=0), (l, va, vb)


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", list(SCENES))
def test_numpy_setup_equals_the_host_walk(name, inv_depth, stereo):
    s = LC.make_scene(inv_depth=inv_depth, **SCENES[name])
    hm = LC.build_host(s, stereo=stereo)
    want = hm.setup_range_ba(s["ini"], s["n"], kf_obs_max=s["n"], min_obs=0)
    got, _ = LR.setup(LC.snapshot(s), s["ini"], s["n"], 1 if stereo else 2, inv_depth)
    assert_same_problem(want, got, inv_depth)
    assert np.array_equal(hm.bad_lmids(), got["bad_lmid"])
    live = [int(k) for k in got["pose_kfid"] if s["ini"] <= k <= s["n"]]
    ncst = 1 if stereo else 2
    assert {int(k) for k, c in zip(got["pose_kfid"], got["pose_const"]) if c and s["ini"] <= k <= s["n"]} == set(live[:ncst])
    if name == "empty":
        assert len(got["res_type"]) == 0 and len(got["pose_kfid"]) == 0
    elif name == "one":   # the one keyframe of the range is constant: a pose, no landmark, no block
        assert len(got["res_type"]) == 0 and list(got["pose_kfid"]) == [s["n"]] and list(got["pose_const"]) == [1]
    else:
        assert len(got["res_type"]) > 0
    if name == "removed":   # constness goes to the next live keyframes of the range
        assert set(live[:ncst]) == ({5} if stereo else {5, 6}) and 3 not in got["pose_kfid"] and 4 not in got["pose_kfid"]


def test_the_scenes_give_the_propagation_landmarks_to_move():
    for name in ("12kf", "70kf"):
        s = LC.make_scene(inv_depth=True, **SCENES[name])
        d = LC.snapshot(s)
        _, oldest, _ = LR.observers(d)
        # 12 keyframes: at least 40 landmarks taken; the 70-keyframe map has fewer than 40 landmarks that a younger keyframe sees
        assert len(s["prop_lm"]) >= (40 if name == "12kf" else 20), (name, len(s["prop_lm"]))
        assert int(np.sum(oldest > s["n"])) >= 20, name
        assert int(np.sum(d["kf_state"][s["n"] + 1:])) >= (5 if name == "70kf" else 3)


@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", ["12kf", "70kf"])
def test_numpy_update_equals_apply_loose_ba(name, inv_depth):
    """crafted "solved" poses / landmarks and flags through Optimizer::applyLooseBA (hash-map objects) and through the six
    numpy steps on the table snapshot: the same surviving keyframes, landmarks, observations, states and stereo flags, poses
    and points equal to rounding (two spellings of the same few SE(3) products: 1e-12 absolute on a 10 m scene)"""
    s = LC.make_scene(inv_depth=inv_depth, **SCENES[name])
    hm, href = LC.build_host(s), LC.build_host(s)
    hpb = href.setup_range_ba(s["ini"], s["n"], kf_obs_max=s["n"], min_obs=0)
    npb, d1 = LR.setup(LC.snapshot(s), s["ini"], s["n"], 1, inv_depth)
    cs = LC.crafted(s, npb)
    Th = hm.apply_loose_ba(s["ini"], s["n"], *LC.in_order(hpb, cs))
    assert Th is not None
    d2, cnt, Tn = LR.update(d1, npb, *LC.in_order(npb, cs), s["n"], s["cur_kfid"], s["P"].calib_l, inv_depth)
    assert np.allclose(LR.mat(Th), Tn, rtol=0, atol=1e-12)
    kf_h, lm_h, ob_h = hm.export()
    kf_n, lm_n, ob_n = LR.canonical(d2)
    assert sorted(kf_h) == sorted(kf_n)
    for k in kf_h:
        assert np.allclose(LR.mat(np.array(kf_h[k])), kf_n[k], rtol=0, atol=1e-12), k
    assert sorted(lm_h) == sorted(lm_n), "surviving landmarks differ"
    for l in lm_h:
        assert lm_h[l][1] == lm_n[l][1], (l, lm_h[l][1], lm_n[l][1])
        assert np.allclose(lm_h[l][0], lm_n[l][0], rtol=0, atol=1e-11), l
    assert ob_h == ob_n, "surviving observations / stereo flags differ"
    # every branch of the update ran: the landmark half of the propagation above all
    assert cnt["n_propagated"] >= 20
    assert cnt["n_kf_younger"] >= 3 and cnt["n_written"] > 100
    assert cnt["n_removed_obs"] > 0 and cnt["n_stereo_off"] > 0 and cnt["n_removed_lm"] > 0
    assert cnt["n_flagged_left"] > 0 and cnt["n_flagged_right"] > 0
    moved = [l for l in s["prop_lm"] if int(l) in lm_n and not np.array_equal(lm_n[int(l)][0], LC.snapshot(s)["lm_xyz"][l])]
    assert len(moved) >= 20


def test_a_range_without_residual_blocks_is_a_no_op():
    s = LC.make_scene(inv_depth=True, **SCENES["empty"])
    hm = LC.build_host(s)
    before = hm.export()
    assert hm.apply_loose_ba(s["ini"], s["n"], np.zeros((0, 7)), np.zeros((0, 1)), np.zeros(0, np.uint8)) is None
    after = hm.export()
    assert before[0] == after[0] and before[2] == after[2]
    pb, d1 = LR.setup(LC.snapshot(s), s["ini"], s["n"], 1, True)
    d2, cnt, _ = LR.update(d1, pb, np.zeros((0, 7)), np.zeros((0, 1)), np.zeros(0), s["n"], s["cur_kfid"], s["P"].calib_l, True)
    assert cnt["ran"] == 0 and all(np.array_equal(d1[k], d2[k]) for k in d1)


def flat_problem(P, pb):
    """the problem `pb` (ids) as a BaProblem in pb's own row order"""
    pidx = {int(k): i for i, k in enumerate(pb["pose_kfid"])}
    lidx = {int(l): i for i, l in enumerate(pb["lm_lmid"])}
    return T.BaProblem(P.calib_l, P.calib_r, np.asarray(P.T_rl, np.float64), P.inv_depth, pb["pose"].copy(), pb["pose_const"],
                       pb["lm"].copy(), np.array([pidx[int(k)] for k in pb["lm_anchor_kfid"]], np.int32) if P.inv_depth else None,
                       pb["lm_anchor_uv"] if P.inv_depth else None, pb["res_type"],
                       np.array([pidx[int(k)] for k in pb["res_kfid"]], np.int32),
                       np.array([lidx[int(l)] for l in pb["res_lmid"]], np.int32), pb["res_uv"])


def loose_options(oracle):
    o = oracle.ba_default_options()
    o.max_iters, o.function_tolerance, o.l2_refine = 5, 1e-4, 0
    return o


@pytest.mark.parametrize("inv_depth", [True, False])
@pytest.mark.parametrize("name", ["12kf", "70kf"])
def test_whole_statement_scenes_are_well_conditioned(oracle, name, inv_depth):
    """what the GPU whole-statement test relies on: every block's chi2 lies at least 1e-6 (relative) away from the threshold,
    so another row order cannot flip a flag; and the spread between the host's and the mirror's row order of one problem,
    solved by the CPU oracle with looseBA's options, stays below the cap / 100 (printed: LOOSE_TOL of the GPU test and
    DESIGN.md section 7 quote it)"""
    s = LC.make_scene(inv_depth=inv_depth, **SCENES[name])
    hpb = LC.build_host(s).setup_range_ba(s["ini"], s["n"], kf_obs_max=s["n"], min_obs=0)
    npb, _ = LR.setup(LC.snapshot(s), s["ini"], s["n"], 1, inv_depth)
    o = loose_options(oracle)
    Qh, Qn = flat_problem(s["P"], hpb), flat_problem(s["P"], npb)
    Rh, Rn = oracle.ba_solve(Qh, o), oracle.ba_solve(Qn, o)
    chi2 = np.asarray(Rh.chi2)
    margin = float(np.min(np.abs(chi2 - o.chi2_th) / o.chi2_th))
    assert margin >= 1e-6, margin
    assert Rh.c.n_outliers_pass1 == Rn.c.n_outliers_pass1 > 0
    ph = {int(k): p for k, p in zip(hpb["pose_kfid"], Qh.pose)}
    pn = {int(k): p for k, p in zip(npb["pose_kfid"], Qn.pose)}
    lh = {int(l): v for l, v in zip(hpb["lm_lmid"], Qh.lm)}
    ln = {int(l): v for l, v in zip(npb["lm_lmid"], Qn.lm)}
    dp = max(float(np.max(np.abs(LR.mat(ph[k]) - LR.mat(pn[k])))) for k in ph)
    dl = max(float(np.max(np.abs(lh[l] - ln[l]) / np.maximum(np.abs(lh[l]), 1e-300))) for l in lh)
    print(f"loose BA row-order spread {name} inv={inv_depth}: poses {dp:.2e}, points {dl:.2e} relative, chi2 margin {margin:.2e}, "
          f"flagged {Rh.c.n_outliers_pass1} of {len(chi2)}")
    assert 100 * dp <= 1e-9 and 100 * dl <= 1e-9, (dp, dl)
