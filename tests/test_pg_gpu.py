"""GPU parity tests (through the C ABI) of ov2_pose_graph_solve against the CPU oracle (oracle/ov2_oracle_pg.c: dense
normal equations there, block-tridiagonal runs on the GPU).  Bar: identical iteration logs (accept / reject, termination),
costs to 1e-9 relative, poses to 1e-8."""
import numpy as np
import pytest

import pg_cases
from ov2slam_amd import ba_types as T, pose_graph
from test_oracle_pg import chain, expm, hat6, mat, pose7

pytestmark = pytest.mark.gpu


def _same_cost(a, b):
    """1e-9 relative; a NaN cost (a NaN measurement) must be NaN on both sides"""
    return bool(np.isnan(a)) and bool(np.isnan(b)) if np.isnan(a) or np.isnan(b) else a == pytest.approx(b, rel=1e-9, abs=1e-18)


def _compare(Pg, Rg, Pc, Rc):
    assert Rg.termination == Rc.termination and Rg.n_log == Rc.n_log
    for a, b in zip(Rg.log[:Rg.n_log], Rc.log[:Rc.n_log]):
        assert (a.step_is_valid, a.step_is_successful) == (b.step_is_valid, b.step_is_successful)
        assert _same_cost(a.cost, b.cost), (a.cost, b.cost)
        assert a.radius == pytest.approx(b.radius, rel=1e-6)
    assert _same_cost(Rg.final_cost, Rc.final_cost), (Rg.final_cost, Rc.final_cost)
    assert np.abs(Pg.pose - Pc.pose).max() < 1e-8
    const = Pc.pose_const != 0
    assert np.array_equal(Pg.pose[const], Pc.pose[const])


@pytest.mark.parametrize("n,drift", [(8, 0.01), (40, 0.01), (200, 0.003)])
def test_local_pose_graph_matches_oracle(ctx, oracle, n, drift):
    """Optimizer::localPoseGraph: loop keyframe constant, odometry chain, one loop edge, 10 iterations at 1e-4"""
    P, gt = chain(np.random.default_rng(n), n, drift=drift)
    Pc = P.copy()
    Rg = pose_graph.solve(ctx, P)
    Rc = oracle.pose_graph_solve(Pc)
    _compare(P, Rg, Pc, Rc)
    assert Rg.final_cost < 0.5 * Rg.initial_cost


def test_full_pose_graph_runs_between_constant_keyframes(ctx, oracle):
    """Optimizer::fullPoseGraph: every frame a pose, keyframes constant, edges between consecutive frames: independent
    runs of free poses, 100 iterations at 1e-6"""
    rng = np.random.default_rng(7)
    n = 300
    gt = [np.eye(4)]
    for k in range(1, n):
        gt.append(gt[-1] @ expm(hat6(np.array([0.1, 0.004, 0.0, 0.0, 0.02, 0.004]))))
    const = np.zeros(n, np.uint8)
    const[::9] = 1
    const[-1] = 1
    est = [gt[k] if const[k] else gt[k] @ expm(hat6(rng.normal(0, 0.01, 6))) for k in range(n)]
    meas = [pose7(np.linalg.inv(gt[k - 1]) @ gt[k] @ expm(hat6(rng.normal(0, 0.001, 6)))) for k in range(1, n)]
    P = T.PgProblem(np.stack([pose7(M) for M in est]), const, np.arange(n - 1), np.arange(1, n), np.stack(meas))
    Pc = P.copy()
    o = pose_graph.default_options(100, 1e-6)
    Rg = pose_graph.solve(ctx, P, o)
    Rc = oracle.pose_graph_solve(Pc, oracle.pg_default_options(100, 1e-6))
    _compare(P, Rg, Pc, Rc)
    err0 = max(np.linalg.norm(mat(pose7(est[k]))[:3, 3] - gt[k][:3, 3]) for k in range(n))
    err1 = max(np.linalg.norm(mat(P.pose[k])[:3, 3] - gt[k][:3, 3]) for k in range(n))
    assert err1 < 0.5 * err0


def test_pose_graph_edge_cases(ctx, oracle):
    # dead reckoning satisfies every odometry edge: nothing moves
    P, _ = chain(np.random.default_rng(2), 12, drift=0.01, loop=False)
    x0 = P.pose.copy()
    R = pose_graph.solve(ctx, P)
    assert R.final_cost < 1e-20 and np.allclose(P.pose, x0, atol=1e-12)
    # every pose constant / no edge: skipped
    Q, _ = chain(np.random.default_rng(2), 6)
    Q.pose_const[:] = 1
    assert pose_graph.solve(ctx, Q).termination == 6
    # an edge between free poses that are not neighbours of the chain is refused, not mis-solved
    B, _ = chain(np.random.default_rng(3), 10)
    B.edge_i = np.append(B.edge_i, 2).astype(np.int32)
    B.edge_j = np.append(B.edge_j, 7).astype(np.int32)
    B.T_ij = np.vstack([B.T_ij, B.T_ij[:1]])
    with pytest.raises(Exception):
        pose_graph.solve(ctx, B)
    # a constant pose in the middle splits the chain into two runs
    S, _ = chain(np.random.default_rng(4), 20)
    S.pose_const[10] = 1
    Sc = S.copy()
    _compare(S, pose_graph.solve(ctx, S), Sc, oracle.pose_graph_solve(Sc))


@pytest.mark.parametrize("case", pg_cases.cases(), ids=pg_cases.ids())
def test_case_matches_oracle(ctx, oracle, case):
    """every case of pg_cases.py (rejected and invalid steps, each termination, the log cap, no Jacobi scaling, the
    quaternion branches of the SE(3) log, the graph shapes, 255 / 256 / 257 runs): one launch each, the bar of this file.
    tests/test_pg_cases_cpu.py holds each case to its branch and to tameness on the oracle."""
    Pc, Rc = pg_cases.reference(oracle, case)
    P = case.problem.copy()
    Rg = pose_graph.solve(ctx, P, pg_cases.apply_options(pose_graph.default_options(), case.options))
    assert pg_cases.flags(Rg) == pg_cases.flags(Rc)
    assert _same_cost(Rg.initial_cost, Rc.initial_cost), (Rg.initial_cost, Rc.initial_cost)
    _compare(P, Rg, Pc, Rc)
    # the model's predicted decrease, from the residuals, jacobians and step of that round: after a rejected step it is
    # only right if the residuals at x were put back.  1e-6 as the radius, which follows from it.
    for k, (a, b) in enumerate(zip(Rg.log[:Rg.n_log], Rc.log[:Rc.n_log])):
        assert a.model_cost_change == pytest.approx(b.model_cost_change, rel=1e-6, abs=0), k
    for k in np.flatnonzero(case.problem.pose_const == 0):       # every run, pose by pose
        assert np.abs(P.pose[k] - Pc.pose[k]).max() < 1e-8, k
    if case.expect.get("unchanged"):        # MIN_RADIUS, no iteration, a rejected only step, FAILURE
        assert np.array_equal(P.pose, case.problem.pose)
