"""GPU tests of the two-view pose refinement (ov2_relpose_refine_batch, csrc/relpose.hip) against the numpy checker
tests/relpose_ref.py.  Bar (that of tests/test_pnp_gpu.py for the sibling kernel): status, LM iteration count and termination
identical, costs within 1e-9 relative, R and t within 1e-9.  The scenes are those of tests/relpose_cases.py, whose tameness
tests/test_relpose_ref_cpu.py checks."""
import numpy as np
import pytest

import relpose_cases as RC
import relpose_ref as RR
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

pytestmark = pytest.mark.gpu
OV2_ERR_INVALID = -1


def _run(mvg, cases, with_skip=True):
    """one batched call.  with_skip: the call carries a mask (all-zero for the frames that have none); otherwise NULL"""
    sk = [np.zeros(len(c["f1"]), np.uint8) if c["skip"] is None else c["skip"] for c in cases] if with_skip else None
    return mvg.refine5pt_batch([c["f1"] for c in cases], [c["f2"] for c in cases], np.array([c["K"] for c in cases]),
                               np.array([c["R0"] for c in cases]), np.array([c["t0"] for c in cases]), RC.MAX_ITERS, sk)


def _frame(r, b):
    return {k: v[b] for k, v in r.items()}


def _same_as_ref(g, e, c):
    assert g["status"] == e["status"]
    assert (g["info"][0], g["info"][1]) == (e["iters"], e["term"])
    for k in range(2):
        assert abs(g["cost"][k] - e["cost"][k]) <= 1e-9 * abs(e["cost"][k])
    if e["status"] == 1:
        assert np.abs(g["R"].ravel() - e["R"]).max() < 1e-9 and np.abs(g["t"] - e["t"]).max() < 1e-9
    else:
        assert g["R"].tobytes() == c["R0"].tobytes() and g["t"].tobytes() == c["t0"].tobytes()


def _bytes(f):
    return tuple(f[k].tobytes() for k in ("R", "t", "info", "cost")) + (int(f["status"]),)


@pytest.fixture(scope="module")
def edge(ctx):
    """the edge batch, run once"""
    return _run(MultiViewGeometry(ctx), RC.edge_batch())


# ---- 1. batch of edge sizes ---------------------------------------------------------------------------------------------
def test_edge_sizes_match_checker(edge):
    cases, refs = RC.edge_batch(), RC.edge_refs()
    assert [int((c["skip"] == 0).sum()) if c["skip"] is not None else len(c["f1"]) for c in cases] == RC.EDGE_N
    for b, (c, e) in enumerate(zip(cases, refs)):
        g = _frame(edge, b)
        print(f"n {RC.EDGE_N[b]}: status {g['status']}, info {g['info'].tolist()}, cost {g['cost'].tolist()}; checker "
              f"{e['status']}, {e['iters']}, {e['term']}, {e['cost']}")
        _same_as_ref(g, e, c)
    # the frames above the minimum do refine; the minimum itself is a determined system and may or may not move
    assert all(edge["status"][b] == 1 for b, n in enumerate(RC.EDGE_N) if n >= 10)


def test_below_the_minimum_is_untouched(edge):
    for b in (0, 1):
        assert RC.EDGE_N[b] < RR.MIN_PAIRS
        c = RC.edge_batch()[b]
        assert edge["status"][b] == 0 and edge["info"][b].tolist() == [0, RR.TERM_SKIPPED]
        assert edge["R"][b].tobytes() == c["R0"].tobytes() and edge["t"][b].tobytes() == c["t0"].tobytes()


def test_refined_pose_is_a_pose(edge):
    for b in np.flatnonzero(edge["status"] == 1):
        R, t = edge["R"][b], edge["t"][b]
        assert np.linalg.norm(R @ R.T - np.eye(3)) < 1e-10 and abs(np.linalg.norm(t) - 1.0) < 1e-15
        assert edge["cost"][b][1] < edge["cost"][b][0]


# ---- 2. batch independence ----------------------------------------------------------------------------------------------
def test_batch_independence(ctx, edge):
    mvg = MultiViewGeometry(ctx)
    cases = RC.edge_batch()
    B = len(cases)
    again = _run(mvg, cases)
    rev = _run(mvg, cases[::-1])
    for b, c in enumerate(cases):
        want = _bytes(_frame(edge, b))
        assert _bytes(_frame(again, b)) == want
        assert _bytes(_frame(rev, B - 1 - b)) == want
        alone = _run(mvg, [c], with_skip=c["skip"] is not None)   # frames without a mask: skip = NULL
        assert _bytes(_frame(alone, 0)) == want


# ---- 3. refusal branches ------------------------------------------------------------------------------------------------
def test_refusals_leave_neighbours_alone(ctx):
    mvg = MultiViewGeometry(ctx)
    cases, refs = RC.refusal_batch(), RC.refusal_refs()
    r = _run(mvg, cases)
    for b, (c, e) in enumerate(zip(cases, refs)):
        _same_as_ref(_frame(r, b), e, c)
    for b in (1, 3):      # exact bearings, NaN in one bearing
        assert r["status"][b] == 0
        assert r["R"][b].tobytes() == cases[b]["R0"].tobytes() and r["t"][b].tobytes() == cases[b]["t0"].tobytes()
    assert r["info"][1].tolist() == [RR.MAX_INVALID, RR.TERM_FAILURE] and r["cost"][1].tolist() == [0.0, 0.0]
    assert r["info"][3].tolist() == [0, RR.TERM_SKIPPED]
    for b in (0, 2, 4):   # the neighbours: refined, and as if they were alone
        assert r["status"][b] == 1
        assert _bytes(_frame(_run(mvg, [cases[b]]), 0)) == _bytes(_frame(r, b))


def _dev_inputs(ctx, f1s, f2s, K):
    n = np.array([len(f) for f in f1s])
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    d = ctx.to_device
    return off, d(off), d(np.concatenate(f1s)), d(np.concatenate(f2s)), d(np.ascontiguousarray(K, np.float64))


def test_in_status_skips_a_frame(ctx):
    mvg = MultiViewGeometry(ctx)
    cases = [RC.refusal_batch()[b] for b in (0, 2, 4)]
    B = len(cases)
    host = _run(mvg, cases)
    off, d_off, d_f1, d_f2, d_K = _dev_inputs(ctx, [c["f1"] for c in cases], [c["f2"] for c in cases], [c["K"] for c in cases])
    d = ctx.to_device
    sk = np.concatenate([np.zeros(len(c["f1"]), np.uint8) if c["skip"] is None else c["skip"] for c in cases])
    R0, t0 = np.array([c["R0"] for c in cases]), np.array([c["t0"] for c in cases])
    d_R, d_t = d(R0), d(t0)
    d_st, d_info, d_cost = d(np.full(B, -7, np.int32)), d(np.full((B, 2), -7, np.int32)), d(np.full((B, 2), -7.0))
    mvg.refine5pt_batch_dev(B, d_off, d_f1, d_f2, d(sk), d_K, RC.MAX_ITERS, d(np.array([2, 0, 1], np.int32)), d_R, d_t,
                            d_st, d_info, d_cost)
    ctx.synchronize()
    assert d_st.get().tolist() == [1, 0, 1]
    assert d_info.get()[1].tolist() == [0, RR.TERM_SKIPPED] and d_cost.get()[1].tolist() == [0.0, 0.0]
    assert d_R.get()[1].tobytes() == R0[1].tobytes() and d_t.get()[1].tobytes() == t0[1].tobytes()
    for b in (0, 2):
        assert d_R.get()[b].tobytes() == host["R"][b].tobytes() and d_t.get()[b].tobytes() == host["t"][b].tobytes()
        assert d_info.get()[b].tobytes() == host["info"][b].tobytes() and d_cost.get()[b].tobytes() == host["cost"][b].tobytes()


# ---- 4. chained _dev form -----------------------------------------------------------------------------------------------
def test_ransac_then_refinement_on_one_stream(ctx):
    """ov2_epipolar_filter_batch_dev then ov2_relpose_refine_batch_dev on the RANSAC's own arrays, no host step between,
    against the two host-pointer calls"""
    mvg = MultiViewGeometry(ctx)
    sc = RC.chain_scenes()
    B = len(sc)
    K = np.array([s["K"] for s in sc])
    seeds = [41 + b for b in range(B)]
    f1s, f2s = [s["bv_kf"] for s in sc], [s["bv_cur"] for s in sc]
    h1 = mvg.compute5ptEssentialMatrix_batch(f1s, f2s, 100, 3.0, K, seeds)
    assert h1["status"].tolist() == [2, 2, 0, 1]
    h2 = mvg.refine5pt_batch(f1s, f2s, K, h1["R"], h1["t"], RC.MAX_ITERS, h1["outlier"])
    assert h2["status"].tolist()[:2] == [1, 1] and h2["status"][2] == 0
    off, d_off, d_f1, d_f2, d_K = _dev_inputs(ctx, f1s, f2s, K)
    d = ctx.to_device
    d_R, d_t = d(np.zeros((B, 9))), d(np.zeros((B, 3)))
    d_out, d_st1 = ctx.empty(int(off[-1]), np.uint8), ctx.empty(B, np.int32)
    d_st2, d_info, d_cost = ctx.empty(B, np.int32), ctx.empty((B, 2), np.int32), ctx.empty((B, 2), np.float64)
    mvg.compute5ptEssentialMatrix_batch_dev(B, d_off, d_f1, d_f2, None, None, None, d_K, 100, 3.0,
                                            d(np.array(seeds, np.uint64)), d_R, d_t, d_out, None, d_st1, None)
    mvg.refine5pt_batch_dev(B, d_off, d_f1, d_f2, d_out, d_K, RC.MAX_ITERS, d_st1, d_R, d_t, d_st2, d_info, d_cost)
    ctx.synchronize()
    assert np.array_equal(d_st1.get(), h1["status"]) and np.array_equal(d_st2.get(), h2["status"])
    assert d_out.get().astype(bool).tobytes() == np.concatenate(h1["outlier"]).tobytes()   # the mask stays the RANSAC's
    assert d_R.get().tobytes() == h2["R"].reshape(B, 9).tobytes() and d_t.get().tobytes() == h2["t"].tobytes()
    assert d_info.get().tobytes() == h2["info"].tobytes() and d_cost.get().tobytes() == h2["cost"].tobytes()
    for b in (0, 1):      # and the refinement did what it is for
        assert RR.dir_err_deg(h2["t"][b], sc[b]["t"]) < RR.dir_err_deg(h1["t"][b], sc[b]["t"])


def test_opt_form_is_ransac_then_refinement(ctx):
    mvg = MultiViewGeometry(ctx)
    s = RC.chain_scenes()[0]
    K = s["K"]
    ok, R, t, idx, refined = mvg.compute5ptEssentialMatrix_opt(s["bv_kf"], s["bv_cur"], 100, 3.0, True, K[0], K[1], seed=41,
                                                              nrefine=RC.MAX_ITERS)
    Kz = np.array([[K[0], K[1], 0., 0.]])
    h1 = mvg.compute5ptEssentialMatrix_batch([s["bv_kf"]], [s["bv_cur"]], 100, 3.0, Kz, [41])
    h2 = mvg.refine5pt_batch([s["bv_kf"]], [s["bv_cur"]], Kz, h1["R"], h1["t"], RC.MAX_ITERS, h1["outlier"])
    assert ok and refined == 1 and idx.tolist() == np.flatnonzero(h1["outlier"][0]).tolist()
    assert R.tobytes() == h2["R"][0].tobytes() and t.tobytes() == h2["t"][0].tobytes()


# ---- 5. argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx):
    c = RC.refusal_batch()[0]
    n = np.array([len(c["f1"])], np.int32)
    f1, f2 = np.ascontiguousarray(c["f1"]), np.ascontiguousarray(c["f2"])
    K = np.ascontiguousarray(c["K"][None])
    R, t = c["R0"].copy(), c["t0"].copy()
    st, info, cost = np.full(1, -7, np.int32), np.full((1, 2), -7, np.int32), np.full((1, 2), -7.0)
    p = lambda a: None if a is None else a.ctypes.data
    call = lambda B, n_, f1_, f2_, K_, it, R_, t_, st_: ctx.lib.ov2_relpose_refine_batch(
        ctx.h, B, p(n_), p(f1_), p(f2_), None, p(K_), it, p(R_), p(t_), p(st_), p(info), p(cost))
    assert call(-1, n, f1, f2, K, 10, R, t, st) == OV2_ERR_INVALID
    assert call(1, n, f1, f2, K, -1, R, t, st) == OV2_ERR_INVALID
    assert call(1, np.array([-3], np.int32), f1, f2, K, 10, R, t, st) == OV2_ERR_INVALID
    for hole in range(7):
        a = [n, f1, f2, K, R, t, st]
        a[hole] = None
        assert call(1, a[0], a[1], a[2], a[3], 10, a[4], a[5], a[6]) == OV2_ERR_INVALID
    # the device form refuses the same before any launch (null device arrays, negative counts)
    dev = lambda B, it, off, R_: ctx.lib.ov2_relpose_refine_batch_dev(ctx.h, B, off, None, None, None, None, it, None, R_,
                                                                      None, None, None, None)
    assert dev(1, 10, None, None) == OV2_ERR_INVALID and dev(-1, 10, None, None) == OV2_ERR_INVALID
    assert dev(1, -1, None, None) == OV2_ERR_INVALID
    assert R.tobytes() == c["R0"].tobytes() and t.tobytes() == c["t0"].tobytes()
    assert (st == -7).all() and (info == -7).all() and (cost == -7.0).all()
    assert ctx.lib.ov2_relpose_refine_batch(ctx.h, 0, None, None, None, None, None, 10, None, None, None, None, None) == 0
