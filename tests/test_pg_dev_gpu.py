"""ov2_pose_graph_solve_batch_dev (csrc/posegraph.hip): the batch solve with poses, T_ij and result records in device memory,
fed from torch device tensors.  Bar: poses, result records and logs are BITWISE equal to ov2_pose_graph_solve_batch on the
same inputs, in a batch of all cases and again with the batch order reversed.

Cases, one per branch family of tests/pg_cases.py, all under WILD_OPTS (38 iterations at 1e-6; one batch has one set of
options): a badly initialised loop that rejects steps (wild9_s5), a two-pose graph (log_x_2.0_3it), the 14-pose graph with
inserted constants (edges between constants, reversed edges, an isolated pose), 257 independent runs (alternating_514: the
runs stride over the 256 threads) and a graph without a free pose (all_constant: skipped)."""
import ctypes as C

import numpy as np
import pytest
import torch     # before the library is loaded: torch brings a HIP runtime of its own and must be the first to arrive

import pg_cases
from ov2slam_amd import pose_graph
from ov2slam_amd.ba_types import PgResultC

pytestmark = pytest.mark.gpu
NAMES = ("wild9_s5", "log_x_2.0_3it", "shapes14_inserted_constants", "alternating_514", "all_constant")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _problems():
    by_name = {c.name: c for c in pg_cases.cases() + pg_cases.legacy_cases()}
    return [by_name[n].problem for n in NAMES]


def _options():
    return pg_cases.apply_options(pose_graph.default_options(), pg_cases.WILD_OPTS)


_HOST = {}


def host_form(ctx):
    """ov2_pose_graph_solve_batch on copies of the cases, once per session: [(solved problem, raw record bytes)]"""
    if "r" not in _HOST:
        Ps = [P.copy() for P in _problems()]
        Rs = pose_graph.solve_batch(ctx, Ps, _options())
        _HOST["r"] = [(P, np.frombuffer(bytes(R), np.uint8), R) for P, R in zip(Ps, Rs)]
    return _HOST["r"]


def dev_form(ctx, order):
    """the device form on the cases in `order`, everything uploaded / downloaded through torch; results in case order"""
    Ps = _problems()
    rec = C.sizeof(PgResultC)
    d_pose = [torch.from_numpy(Ps[k].pose.copy()).cuda() for k in order]
    d_T = [torch.from_numpy(Ps[k].T_ij.copy()).cuda() for k in order]
    # pre-filled with a pattern: the call has to clear the records itself
    d_res = torch.full((len(order) * rec,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pose_graph.solve_batch_dev(ctx, [Ps[k] for k in order], d_pose, d_T, d_res, _options())
    ctx.synchronize()
    res = d_res.cpu().numpy().reshape(len(order), rec)
    out = [None] * len(Ps)
    for slot, k in enumerate(order):
        out[k] = (d_pose[slot].cpu().numpy(), res[slot], d_T[slot].cpu().numpy())
    return out


@pytest.mark.parametrize("rev", [False, True], ids=["in_order", "reversed"])
def test_device_form_is_bitwise_the_host_form(ctx, rev):
    want = host_form(ctx)
    order = list(range(len(NAMES)))[::-1] if rev else list(range(len(NAMES)))
    got = dev_form(ctx, order)
    Ps = _problems()
    for name, P0, (Ph, raw, R), (pose, rec, Tij) in zip(NAMES, Ps, want, got):
        assert np.array_equal(pose.view(np.uint64), Ph.pose.view(np.uint64)), name
        assert np.array_equal(rec, raw), name
        assert np.array_equal(Tij.view(np.uint64), P0.T_ij.view(np.uint64)), name      # the measurements are read only
    by = {n: w[2] for n, w in zip(NAMES, want)}
    # the cases are what they are picked for
    assert by["all_constant"].termination == pg_cases.SKIPPED and by["all_constant"].n_log == 0
    assert "r" in pg_cases.flags(by["wild9_s5"])[:-1]
    assert by["alternating_514"].n_log > 3 and by["log_x_2.0_3it"].n_log > 3
    k = NAMES.index("all_constant")
    assert np.array_equal(got[k][0], Ps[k].pose)


def test_refusals_and_empty_batch(ctx):
    Ps = _problems()[:2]
    d_pose = [torch.from_numpy(P.pose.copy()).cuda() for P in Ps]
    d_T = [torch.from_numpy(P.T_ij.copy()).cuda() for P in Ps]
    d_res = torch.zeros(2 * C.sizeof(PgResultC), dtype=torch.uint8, device="cuda")
    bad = Ps[1].copy()
    bad.edge_j = bad.edge_j.copy()
    bad.edge_j[0] = 9
    with pytest.raises(Exception, match=r"\(-1\).*graph 1"):
        pose_graph.solve_batch_dev(ctx, [Ps[0], bad], d_pose, d_T, d_res)
    ctx.synchronize()
    for P, d in zip(Ps, d_pose):           # nothing was enqueued
        assert np.array_equal(d.cpu().numpy(), P.pose)
    pose_graph.solve_batch_dev(ctx, [], [], [], d_res)      # B = 0: OV2_OK
    assert ctx.lib.ov2_pose_graph_solve_batch_dev(ctx.h, -1, None, None, None) == -1
