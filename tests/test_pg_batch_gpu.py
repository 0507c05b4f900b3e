"""ov2_pose_graph_solve_batch (csrc/posegraph.hip): B chain graphs in one launch, one workgroup per graph.  Bar: every
graph's poses, result and iteration log are bit-identical (raw structs, np.array_equal) to ov2_pose_graph_solve on it,
whatever the batch around it and wherever it stands; every graph also passes the oracle bar of tests/test_pg_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import pg_cases
from ov2slam_amd import pose_graph
from ov2slam_amd.ba_types import PgProblemC, PgResultC
from test_oracle_pg import chain
from test_pg_gpu import _compare

pytestmark = pytest.mark.gpu


def _raw(R):
    return np.frombuffer(bytes(R), np.uint8)


def _case(name):
    by_name = {c.name: c for c in pg_cases.cases() + pg_cases.legacy_cases()}
    return by_name[name]


def default_batch():
    """chains of 2, 8, 40 and 257 poses and the `{}` cases of pg_cases (consistent, all_constant -- skipped, in the middle
    --, split, local_*): all under the default options (10 iterations, 1e-4)"""
    out = [("chain_%d" % n, chain(np.random.default_rng(100 + n), n, drift=0.01)[0]) for n in (2, 8, 40, 257)]
    legacy = {c.name: c for c in pg_cases.legacy_cases() if c.options == {}}
    assert set(legacy) == {"consistent", "all_constant", "split", "local_8", "local_40", "local_200"}
    out[2:2] = [(n, legacy[n].problem) for n in ("consistent", "all_constant", "split")]
    out += [(n, legacy[n].problem) for n in ("local_8", "local_40", "local_200")]
    return out


def wild_batch():
    """under WILD_OPTS: a graph that rejects steps and one that ends in TERM_FAILURE beside healthy ones"""
    names = ("wild9_s5", "wild16_s3", "wild9_nan_failure")
    for n in names:
        assert _case(n).options == pg_cases.WILD_OPTS
    return [(n, _case(n).problem) for n in names] + [("chain_12", chain(np.random.default_rng(12), 12, drift=0.01)[0])]


def _options(overrides):
    return pg_cases.apply_options(pose_graph.default_options(), overrides)


_SINGLE = {}


def single(ctx, key, batch, overrides):
    """every graph of `batch` through ov2_pose_graph_solve, once per session (callers leave the result unchanged)"""
    if key not in _SINGLE:
        out = []
        for _, P in batch:
            Q = P.copy()
            out.append((Q, pose_graph.solve(ctx, Q, _options(overrides))))
        _SINGLE[key] = out
    return _SINGLE[key]


def _solve_batch(ctx, batch, overrides, order=None):
    order = list(range(len(batch))) if order is None else order
    Ps = [batch[k][1].copy() for k in order]
    Rs = pose_graph.solve_batch(ctx, Ps, _options(overrides))
    back = {k: (P, R) for k, P, R in zip(order, Ps, Rs)}
    return [back[k] for k in range(len(batch))]


def _same(batch, got, want):
    for (name, _), (Pb, Rb), (Ps, Rs) in zip(batch, got, want):
        assert np.array_equal(Pb.pose.view(np.uint64), Ps.pose.view(np.uint64)), name
        assert Rb.n_log == Rs.n_log and Rb.termination == Rs.termination, name
        assert np.array_equal(_raw(Rb), _raw(Rs)), name


@pytest.mark.parametrize("which", ["default", "wild"])
def test_batch_is_bitwise_its_single_calls(ctx, which):
    batch, o = (default_batch(), {}) if which == "default" else (wild_batch(), pg_cases.WILD_OPTS)
    want = single(ctx, which, batch, o)
    got = _solve_batch(ctx, batch, o)
    _same(batch, got, want)
    # the same batch reversed: a graph's result does not depend on its position
    _same(batch, _solve_batch(ctx, batch, o, order=list(range(len(batch)))[::-1]), want)
    if which == "default":
        terms = {n: R.termination for (n, _), (_, R) in zip(batch, got)}
        assert terms["all_constant"] == pg_cases.SKIPPED and terms["chain_257"] != pg_cases.SKIPPED
        skipped = [k for k, (n, _) in enumerate(batch) if n == "all_constant"][0]
        assert np.array_equal(got[skipped][0].pose, batch[skipped][1].pose)
    else:
        by = {n: R for (n, _), (_, R) in zip(batch, got)}
        assert by["wild9_nan_failure"].termination == pg_cases.FAILURE
        assert "r" in pg_cases.flags(by["wild9_s5"])[:-1] and "r" in pg_cases.flags(by["wild16_s3"])[:-1]


def test_batch_matches_oracle(ctx, oracle):
    batch = default_batch()
    for (name, P), (Pg, Rg) in zip(batch, _solve_batch(ctx, batch, {})):
        Pc = P.copy()
        Rc = oracle.pose_graph_solve(Pc)
        _compare(Pg, Rg, Pc, Rc)


def test_batch_sizes(ctx):
    P8 = chain(np.random.default_rng(108), 8, drift=0.01)[0]
    Q = P8.copy()
    Rs = pose_graph.solve(ctx, Q)
    one = _solve_batch(ctx, [("chain_8", P8)], {})
    _same([("chain_8", P8)], one, [(Q, Rs)])
    many = [("copy_%d" % k, P8) for k in range(64)]
    _same(many, _solve_batch(ctx, many, {}), [(Q, Rs)] * 64)
    assert Rs.final_cost < 0.5 * Rs.initial_cost


OV2_ERR_INVALID, OV2_ERR_UNSUPPORTED = -1, -5      # include/ov2slam_hip.h


def _call(ctx, B, Ps):
    """the raw status of ov2_pose_graph_solve_batch(B, Ps) and of ov2_pose_graph_solve on each graph's copy"""
    o = pose_graph.default_options()
    pcs = (PgProblemC * len(Ps))(*[P.as_c() for P in Ps])
    rcs = (PgResultC * len(Ps))()
    st = ctx.lib.ov2_pose_graph_solve_batch(ctx.h, B, pcs, C.byref(o), rcs)
    msg = ctx.lib.ov2_last_error(ctx.h)
    singles = []
    for P in Ps:
        pc, r = P.copy().as_c(), PgResultC()
        singles.append(ctx.lib.ov2_pose_graph_solve(ctx.h, C.byref(pc), C.byref(o), C.byref(r)))
    return st, msg, singles


def test_refusals(ctx):
    Ps = [chain(np.random.default_rng(200 + k), 10)[0] for k in range(5)]
    G = Ps[3]      # an edge between free poses that are not neighbours of the chain
    G.edge_i = np.append(G.edge_i, 2).astype(np.int32)
    G.edge_j = np.append(G.edge_j, 7).astype(np.int32)
    G.T_ij = np.vstack([G.T_ij, G.T_ij[:1]])
    before = [P.pose.copy() for P in Ps]
    st, msg, singles = _call(ctx, 5, Ps)
    assert st == OV2_ERR_UNSUPPORTED and singles == [0, 0, 0, OV2_ERR_UNSUPPORTED, 0] and b"graph 3" in msg
    for P, x in zip(Ps, before):       # all five untouched, the four healthy ones included
        assert np.array_equal(P.pose, x)
    with pytest.raises(Exception, match="graph 3"):
        pose_graph.solve_batch(ctx, Ps)
    # an edge index out of range in graph 1: the single call's status as well
    Ps[3] = chain(np.random.default_rng(203), 10)[0]
    Ps[1].edge_j = Ps[1].edge_j.copy()
    Ps[1].edge_j[4] = 10
    st, msg, singles = _call(ctx, 5, Ps)
    assert st == OV2_ERR_INVALID and singles == [0, OV2_ERR_INVALID, 0, 0, 0] and b"graph 1" in msg
    for P, x in zip(Ps, before):
        assert np.array_equal(P.pose, x)
    good = Ps[:1]
    assert pose_graph.solve_batch(ctx, []) == []                                           # B = 0: OV2_OK
    assert ctx.lib.ov2_pose_graph_solve_batch(ctx.h, 0, None, None, None) == 0
    assert _call(ctx, -1, good)[0] == OV2_ERR_INVALID                                       # B < 0
    assert _call(ctx, 65536, good)[0] == OV2_ERR_INVALID                                    # above OV2_PG_MAX_BATCH
    assert np.array_equal(good[0].pose, before[0])


def test_one_launch_per_call(ctx):
    """the context's kernel counters (slot OV2_K_MAP + 6, "pose_graph_kernel"): one launch whatever B is, none when every
    graph is skipped"""
    batch = default_batch()
    Q = _case("all_constant").problem
    ctx.kernel_timing(True)
    try:
        ctx.kernel_times()
        _solve_batch(ctx, batch, {})
        t_many = ctx.kernel_times()
        _solve_batch(ctx, [("a", Q), ("b", Q)], {})
        t_none = ctx.kernel_times()
        for _, P in batch[:3]:
            pose_graph.solve(ctx, P.copy())
        t_single = ctx.kernel_times()
    finally:
        ctx.kernel_timing(False)
    assert t_many["pose_graph_kernel"][1] == 1 and set(t_many) == {"pose_graph_kernel"}
    assert t_none == {}
    assert t_single["pose_graph_kernel"][1] == 3
