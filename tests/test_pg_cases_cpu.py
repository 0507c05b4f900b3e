"""The pose-graph cases of pg_cases.py, held to what they exist for, without a GPU: each reaches its branch on the oracle
(oracle/ov2_oracle_pg.c), each is numerically tame (so that a GPU mismatch in tests/test_pg_gpu.py is a kernel error and
no coin flip), and the oracle's residual on every branch of the SE(3) log agrees with a 50-digit mpmath reference."""
import mpmath as mp
import numpy as np
import pytest

import pg_cases as pc

CASES = pc.cases()
LOG_0IT = [c for c in CASES if "edge" in c.expect and c.options["max_iters"] == 0]
DPS = 50


# ---- each case reaches its branch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=pc.ids())
def test_case_reaches_its_branch(oracle, case):
    P, R = pc.reference(oracle, case)
    e, f = case.expect, pc.flags(R)
    assert f[0] == "A"
    if "termination" in e:
        assert R.termination == e["termination"], (f, R.termination)
    if e.get("rejected"):
        assert "r" in f[:-1], f               # the closing FUNCTION_TOLERANCE entry is logged unsuccessful too: not counted
    if "flags" in e:
        assert f == e["flags"]
    if "n_log" in e:
        assert R.n_log == e["n_log"]
    if "min_accepted" in e:
        assert f[1:].count("A") >= e["min_accepted"], f
        assert R.final_cost < R.initial_cost
    if e.get("unchanged"):
        assert np.array_equal(P.pose, case.problem.pose)
    else:
        free = case.problem.pose_const == 0
        assert not np.array_equal(P.pose[free], case.problem.pose[free])
    if "isolated" in e:
        k = e["isolated"]
        assert not case.problem.pose_const[k] and k not in case.problem.edge_i and k not in case.problem.edge_j
        assert np.array_equal(P.pose[k], case.problem.pose[k])
    const = case.problem.pose_const != 0
    assert np.array_equal(P.pose[const], case.problem.pose[const])
    if e.get("tame", True):
        assert np.isfinite(R.final_cost) and R.final_cost > 1e-6     # no case ends on the rounding floor


def _graph(P):
    """(nf, n_edge, lengths of the runs of coupled free poses) as ov2_pose_graph_solve splits them"""
    fidx = np.cumsum(P.pose_const == 0) - 1
    fidx[P.pose_const != 0] = -1
    nf = int((P.pose_const == 0).sum())
    couple = np.zeros(nf, bool)
    for i, j in zip(fidx[P.edge_i], fidx[P.edge_j]):
        if i >= 0 and j >= 0:
            assert abs(i - j) == 1
            couple[min(i, j)] = True
    lengths, run = [], 1
    for f in range(nf):
        if f + 1 < nf and couple[f]:
            run += 1
        else:
            lengths.append(run); run = 1
    return nf, len(P.edge_i), lengths


def test_case_set_covers_the_terminations_and_shapes():
    by = {c.name: c for c in CASES}
    assert {c.expect.get("termination") for c in CASES} >= {pc.MAX_ITER, pc.FTOL, pc.PTOL, pc.GTOL, pc.MIN_RADIUS, pc.FAILURE}
    assert any(c.options.get("jacobi_scaling") == 0 and c.expect.get("rejected") for c in CASES)
    assert by["wild9_log_cap"].options["max_iters"] > by["wild9_log_cap"].expect["n_log"] == 40
    # the three quaternion branches below trace 0, each at 3.0 and at pi - 1e-6, and at exactly pi
    for ang in (3.0, np.pi - 1e-6, np.pi):
        assert {c.expect["quat_branch"] for c in LOG_0IT if c.expect["edge"][1] == ang} == {"x", "y", "z"}
    assert {c.expect["edge"][1] for c in LOG_0IT if c.expect.get("series")} == {1e-11, 0.0}
    # sizes either side of the 256 threads that edges, pose blocks and runs are strided over
    g = {n: _graph(by["alternating_%d" % n].problem) for n in (511, 513, 514)}
    assert [(g[n][0], g[n][1], len(g[n][2])) for n in (511, 513, 514)] == [(255, 510, 255), (256, 512, 256), (257, 513, 257)]
    g = {n: _graph(by["alternating_%d_left_edges" % n].problem) for n in (511, 513, 514)}
    assert [(g[n][0], g[n][1]) for n in (511, 513, 514)] == [(255, 255), (256, 256), (257, 257)]
    assert _graph(by["mixed_runs"].problem)[2] == [1, 2, 3, 4, 5, 1, 3]
    # shapes14: edges between constants, a constant on either side, reversed edges, a doubled edge, an isolated free pose
    S = by["shapes14"].problem
    ci, cj = S.pose_const[S.edge_i] != 0, S.pose_const[S.edge_j] != 0
    assert (ci & cj).sum() == 2 and (ci & ~cj).any() and (~ci & cj).any()
    assert (S.edge_i > S.edge_j).sum() == 4
    assert any(S.pose_const[i] and not S.pose_const[j] for i, j in zip(S.edge_i, S.edge_j) if i > j)
    pairs = [tuple(sorted(p)) for p in zip(S.edge_i, S.edge_j)]
    assert pairs.count((2, 3)) == 2
    assert _graph(S)[2] == [4, 6, 1]
    Q = by["shapes14_inserted_constants"].problem
    free = np.flatnonzero(Q.pose_const == 0)
    assert (free != np.arange(len(free)) + 1).any() and _graph(Q)[2] == [4, 6, 1]
    N = by["shapes14_scaled_quaternions"].problem
    assert np.allclose(np.abs(np.linalg.norm(N.pose[:, 3:], axis=1) - 1), 1e-3, rtol=1e-6)
    assert np.allclose(np.abs(np.linalg.norm(N.T_ij[:, 3:], axis=1) - 1), 1e-3, rtol=1e-6)


# ---- each case is tame ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c.expect.get("tame", True)],
                         ids=[c.name for c in CASES if c.expect.get("tame", True)])
def test_case_is_tame(oracle, case):
    """five copies with the free translations scaled by 1 +- 1e-13: the same log and termination, costs to 1e-11
    relative, poses to 1e-10, model cost changes to 1e-8 (100 x under the GPU bars of 1e-9, 1e-8 and 1e-6).  A condition on the inputs: a case that
    fails it is replaced, never the bound.  Measured: costs <= 1.4e-12, poses <= 4e-13 (the perturbation itself)."""
    P0, R0 = pc.reference(oracle, case)
    rng = np.random.default_rng(1)
    free = case.problem.pose_const == 0
    for _ in range(5):
        Q = case.problem.copy()
        Q.pose[free, :3] *= 1.0 + 1e-13 * rng.choice([-1.0, 1.0], (int(free.sum()), 3))
        P, R = pc.solve_oracle(oracle, case, Q)
        assert pc.flags(R) == pc.flags(R0) and R.termination == R0.termination
        for a, b in zip(R.log[:R.n_log], R0.log[:R0.n_log]):
            assert a.cost == pytest.approx(b.cost, rel=1e-11, abs=0)
            assert a.model_cost_change == pytest.approx(b.model_cost_change, rel=1e-8, abs=0)    # GPU bar 1e-6; measured 5e-10
        assert R.initial_cost == pytest.approx(R0.initial_cost, rel=1e-11, abs=0)
        assert R.final_cost == pytest.approx(R0.final_cost, rel=1e-11, abs=0)
        assert np.abs(P.pose - P0.pose).max() < 1e-10


# ---- the oracle's residual against mpmath ---------------------------------------------------------------------------------

def _mp_pose(p7):
    t, q = [mp.mpf(float(v)) for v in p7[:3]], [mp.mpf(float(v)) for v in p7[3:]]
    n = mp.sqrt(sum(v * v for v in q))
    x, y, z, w = [v / n for v in q]
    M = mp.eye(4)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    for i in range(3):
        for j in range(3):
            M[i, j] = R[i][j]
        M[i, 3] = t[i]
    return M


def _mp_hat6(r):
    H = mp.zeros(4)
    H[0, 1], H[0, 2], H[1, 0], H[1, 2], H[2, 0], H[2, 1] = -r[5], r[4], r[5], -r[3], -r[4], r[3]
    H[0, 3], H[1, 3], H[2, 3] = r[0], r[1], r[2]
    return H


def _mp_residual_transform(P):
    """Tj^-1 Ti Tij of the single edge, from the doubles the solvers get"""
    return mp.inverse(_mp_pose(P.pose[P.edge_j[0]])) * _mp_pose(P.pose[P.edge_i[0]]) * _mp_pose(P.T_ij[0])


def _mp_se3_log(E):
    """closed-form principal log [rho, omega] of E: angle from atan2 of the antisymmetric part and the trace, rho from
    V(omega) rho = t.  At exactly pi the antisymmetric part vanishes and the sign of omega is free: the axis of the
    largest diagonal entry, negative (Sophus: qw == 0 takes -pi)"""
    v = [(E[2, 1] - E[1, 2]) / 2, (E[0, 2] - E[2, 0]) / 2, (E[1, 0] - E[0, 1]) / 2]     # sin(theta) axis
    s, c = mp.sqrt(sum(a * a for a in v)), (E[0, 0] + E[1, 1] + E[2, 2] - 1) / 2
    theta = mp.atan2(s, c)
    if s == 0 and c < 0:
        k = max(range(3), key=lambda i: E[i, i])
        col = [(E[i, k] + (1 if i == k else 0)) / 2 for i in range(3)]
        nrm = mp.sqrt(sum(a * a for a in col))
        om = [-mp.pi * a / nrm for a in col]
    elif s == 0:
        om = [mp.mpf(0)] * 3
    else:
        om = [theta * a / s for a in v]
    O = mp.matrix([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    th2 = sum(a * a for a in om)
    if th2 == 0:
        V = mp.eye(3)
    else:
        th = mp.sqrt(th2)
        V = mp.eye(3) + (1 - mp.cos(th)) / th2 * O + (th - mp.sin(th)) / (th2 * th) * O * O
    rho = mp.lu_solve(V, mp.matrix([E[0, 3], E[1, 3], E[2, 3]]))
    return [rho[0], rho[1], rho[2]] + om


def _max_abs(M):
    return max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))


@pytest.mark.parametrize("case", LOG_0IT, ids=[c.name for c in LOG_0IT])
def test_oracle_residual_against_mpmath(oracle, case):
    """mp.logm leaves the principal branch close to pi, so the inverse is what is checked everywhere: exp(hat(r))
    reproduces Tj^-1 Ti Tij to 1e-12 with |omega| <= pi; below 3.0 rad also r against mp.logm to 1e-12; and the solver's
    initial cost is 0.5 |r|^2 of the closed-form log to 1e-12 relative"""
    P = case.problem
    axis, angle = case.expect["edge"]
    r, _, _ = oracle.pg_eval_edge(P.pose[0], P.pose[1], P.T_ij[0], want_jac=False)
    with mp.workdps(DPS):
        E = _mp_residual_transform(P)
        # the case is on the branch it is named for
        tr = E[0, 0] + E[1, 1] + E[2, 2]
        branch = "tr" if tr > 0 else "xyz"[max(range(3), key=lambda i: E[i, i])]
        assert branch == case.expect["quat_branch"]
        assert _max_abs(mp.expm(_mp_hat6([mp.mpf(float(v)) for v in r])) - E) < 1e-12
        assert np.linalg.norm(r[3:]) <= np.pi
        ref = _mp_se3_log(E)
        assert _max_abs(mp.expm(_mp_hat6(ref)) - E) < 1e-30        # the reference is a log of E (50 digits, less cancellation)
        assert abs(mp.sqrt(sum(a * a for a in ref[3:])) - angle) < 1e-12
        if case.expect.get("series"):
            assert mp.sqrt(sum(a * a for a in ref[3:])) < 2e-10
        if angle < 3.0:
            L = mp.logm(E)
            lg = [L[0, 3], L[1, 3], L[2, 3], L[2, 1], L[0, 2], L[1, 0]]
            assert max(abs(mp.re(a) - float(b)) for a, b in zip(lg, r)) < 1e-12
            assert max(abs(mp.re(a) - b) for a, b in zip(lg, ref)) < 1e-25
        assert max(abs(a - float(b)) for a, b in zip(ref, r)) < 1e-12
        cost = float(sum(a * a for a in ref) / 2)
    _, R = pc.reference(oracle, case)
    assert R.initial_cost == pytest.approx(cost, rel=1e-12, abs=0)
    if angle == np.pi:
        assert np.array_equal(r[3:], -np.pi * np.eye(3)["xyz".index(axis)])
        assert cost == pytest.approx(0.5 * (float(r[:3] @ r[:3]) + np.pi ** 2), rel=1e-14)
