"""Seeded pose-graph problems that reach every branch of the LM loop and of the SE(3) log which ov2_pose_graph_solve
(csrc/posegraph.hip) and its CPU restatement (oracle/ov2_oracle_pg.c) share: rejected and invalid steps, every
termination, the log cap, the quaternion branches of residual rotations past 120 degrees, and the graph shapes of
Optimizer::fullPoseGraph (reversed edges, edges between constants, hundreds of independent runs).

A case is (name, problem, options, expect): `options` overrides fields of the default options (10 iterations at 1e-4),
`expect` names what the case exists for.  tests/test_pg_cases_cpu.py holds every case to its `expect` on the oracle and
checks that it is numerically tame; tests/test_pg_gpu.py compares the GPU solve of the same case; scripts/oracle_cov.py
runs them through a coverage build of the oracle.  Keys of `expect`:
  termination   ba_types.TERM code the solve ends on
  rejected      at least one valid, unsuccessful step before the last log entry
  flags         the whole accept (A) / reject (r) / invalid (i) string of the log
  n_log         number of log entries
  min_accepted  at least this many accepted steps (the first log entry, the start point, not counted)
  unchanged     the poses come back bitwise as they went in
  isolated      index of a free pose without any edge: comes back bitwise
  tame          False: exempt from the perturbation check (NaN costs; a sign that hangs on qw == 0 exactly)
  edge          group d: (axis, angle) of the residual rotation of the single edge
  series        group d: the rotation is below the 2e-10 under which the log takes its small-angle series
  quat_branch   group d: branch of the rotation-matrix -> quaternion conversion ("tr", "x", "y", "z")"""
from collections import namedtuple

import numpy as np
from scipy.linalg import expm

from ov2slam_amd import ba_types as T
from test_oracle_pg import chain, hat6, mat, pose7

MAX_ITER, FTOL, PTOL, GTOL, MIN_RADIUS, FAILURE, SKIPPED = range(7)
Case = namedtuple("Case", "name problem options expect")

RHO = np.array([0.3, -0.2, 0.5])     # translation of every group-d residual transform


def apply_options(o, overrides):
    """sets the overridden fields on an options struct of either side (the oracle's or the product's defaults)"""
    for k, v in overrides.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def flags(R):
    """the log as a string: A accepted, r valid but unsuccessful (incl. the closing FUNCTION_TOLERANCE entry), i invalid"""
    return "".join("i" if not e.step_is_valid else ("A" if e.step_is_successful else "r") for e in R.log[:R.n_log])


def solve_oracle(oracle, case, problem=None):
    """solves a copy of the case's problem (or of `problem`) on the oracle; returns (solved copy, result)"""
    P = (case.problem if problem is None else problem).copy()
    R = oracle.pose_graph_solve(P, apply_options(oracle.pg_default_options(), case.options))
    return P, R


_REFERENCE = {}


def reference(oracle, case):
    """the oracle's solve of the case, computed once per session and shared (callers leave it unchanged)"""
    if case.name not in _REFERENCE:
        _REFERENCE[case.name] = solve_oracle(oracle, case)
    return _REFERENCE[case.name]


def run(case, oracle):
    """what scripts/oracle_cov.py calls for every case"""
    return solve_oracle(oracle, case)


# ---- a. badly initialised loops -------------------------------------------------------------------------------------

def wild(n, rot, seed):
    """the arc of test_oracle_pg.chain with exact odometry and the loop edge (0, n - 1); pose 0 constant; the estimates
    are far off: gt[k] exp([N(0, 1) x 3, N(0, rot) x 3])"""
    rng = np.random.default_rng(seed)
    P, gt = chain(rng, n, drift=0.0)      # draws the (zero) measurement noise first
    for k in range(1, n):
        P.pose[k] = pose7(gt[k] @ expm(hat6(np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, rot, 3)]))))
    return P


WILD_OPTS = dict(max_iters=38, function_tolerance=1e-6)


def _wild_cases():
    W = wild(9, 1.5, 5)
    out = [
        Case("wild9_s5", W, WILD_OPTS, dict(rejected=True, termination=FTOL, min_accepted=3)),
        Case("wild9_s7_30it", wild(9, 1.5, 7), dict(WILD_OPTS, max_iters=30),
             dict(rejected=True, termination=MAX_ITER, min_accepted=3)),
        Case("wild16_s3", wild(16, 2.5, 3), WILD_OPTS, dict(rejected=True, termination=FTOL, min_accepted=3)),
        # b. one option each on wild(9, 1.5, 5): the tolerance is forced by the option, far above the noise floor
        Case("wild9_ptol", W, dict(WILD_OPTS, parameter_tolerance=1e-2), dict(termination=PTOL, rejected=True)),
        Case("wild9_gtol", W, dict(WILD_OPTS, gradient_tolerance=1e-1), dict(termination=GTOL, rejected=True)),
        Case("wild9_min_radius", W, dict(WILD_OPTS, initial_radius=1e-33),
             dict(termination=MIN_RADIUS, n_log=1, unchanged=True)),
        Case("wild9_0it", W, dict(WILD_OPTS, max_iters=0), dict(termination=MAX_ITER, n_log=1, unchanged=True)),
        Case("wild9_1it", W, dict(WILD_OPTS, max_iters=1), dict(termination=MAX_ITER, flags="Ar", unchanged=True)),
        Case("wild9_no_jacobi", W, dict(WILD_OPTS, jacobi_scaling=0), dict(rejected=True, min_accepted=3)),
        # without scaling the gradient norm after an accepted step comes from the plain -g (PG_NEG in the kernel); only
        # the gradient tolerance reads it
        Case("wild9_no_jacobi_gtol", W, dict(WILD_OPTS, jacobi_scaling=0, gradient_tolerance=1e-1),
             dict(termination=GTOL, rejected=True, min_accepted=3)),
        Case("wild9_log_cap", W, dict(initial_radius=1e-2, max_radius=1.0, max_iters=60, function_tolerance=0.0),
             dict(termination=MAX_ITER, n_log=T.MAX_LOG, flags="A" * T.MAX_LOG)),
    ]
    # c. a NaN measurement: no step is ever valid; bounded by max_consecutive_invalid_steps rounds
    F = W.copy()
    F.T_ij = F.T_ij.copy()               # PgProblem.copy() shares the measurements
    F.T_ij[3, 1] = np.nan
    out.append(Case("wild9_nan_failure", F, WILD_OPTS,
                    dict(termination=FAILURE, flags="Aiiii", unchanged=True, tame=False)))
    return out


# ---- d. one edge, one free pose: the residual log(Tj^-1 Ti Tij) on every branch of the SE(3) log ------------------------

def rotvec(axis, angle):
    a = np.asarray(axis, float)
    return a / np.linalg.norm(a) * angle


def pair(E, identity=False):
    """pose 0 constant, pose 1 free, one edge (0, 1) whose residual transform Tj^-1 Ti Tij is E"""
    if identity:
        Ti = Tj = np.eye(4)
    else:
        Ti = expm(hat6(np.array([0.4, -1.1, 0.7, 0.3, -0.5, 0.2])))
        Tj = expm(hat6(np.array([1.3, 0.2, -0.6, -0.4, 0.1, 0.6])))
    Tij = np.linalg.inv(Ti) @ Tj @ E
    return T.PgProblem(np.stack([pose7(Ti), pose7(Tj)]), np.array([1, 0], np.uint8), [0], [1], np.stack([pose7(Tij)]))


def residual_transform(axis, angle):
    E = np.eye(4)
    E[:3, :3] = expm(hat6(np.concatenate([np.zeros(3), rotvec(axis, angle)])))[:3, :3]
    E[:3, 3] = RHO
    return E


AXES = {"x": (1.0, 0.01, 0.0), "y": (0.0, 1.0, 0.01), "z": (0.01, 0.0, 1.0), "generic": (0.5, -0.6, 0.62)}
# (axis, angle, label); trace(R) = 1 + 2 cos(angle) <= 0 from 120 degrees on
LOG_EDGES = ([(a, ang, lab) for a in "xyz" for ang, lab in ((2.0, "2.0"), (3.0, "3.0"), (np.pi - 1e-6, "pi-1e-6"))] +
             [("generic", 3.1, "3.1"), ("generic", 1e-3, "1e-3"), ("generic", 1e-9, "1e-9"), ("generic", 1e-11, "1e-11"),
              ("generic", 0.0, "0")])


def _log_cases():
    out = []
    for axis, angle, lab in LOG_EDGES:
        E = residual_transform(AXES[axis], angle)
        branch = "tr" if np.trace(E[:3, :3]) > 0 else "xyz"[int(np.argmax(np.diag(E[:3, :3])))]
        P = pair(E)
        for it in (0, 3):
            exp = dict(termination=MAX_ITER, edge=(axis, angle), quat_branch=branch, series=angle < 2e-10)
            if it == 0:
                exp.update(n_log=1, unchanged=True)
            else:      # a unit radius damps the steps: three of them stay far above the rounding floor of this zero-residual problem
                exp.update(flags="AAAA")
            out.append(Case("log_%s_%s_%dit" % (axis, lab, it), P,
                            dict(max_iters=it, function_tolerance=1e-6, initial_radius=1.0), exp))
    # exactly pi: identity poses, measurement quaternion a unit vector: qw == 0, omega = -pi axis
    for k, axis in enumerate("xyz"):
        P = pair(np.eye(4), identity=True)
        P.T_ij[0] = np.array([RHO[0], RHO[1], RHO[2], 0, 0, 0, 0.0])
        P.T_ij[0, 3 + k] = 1.0
        out.append(Case("log_%s_pi_0it" % axis, P, dict(max_iters=0),
                        dict(termination=MAX_ITER, n_log=1, unchanged=True, tame=False, edge=(axis, np.pi), quat_branch=axis)))
    return out


# ---- e. graph shapes -----------------------------------------------------------------------------------------------------

def _inv7(p7):
    return pose7(np.linalg.inv(mat(p7)))


def shapes14():
    """14-pose loop with drift 0.05; poses {0, 5, 6, 13} constant: the edges 5-6 and 0-13 join two constants, 4-5 has
    the constant on the edge_j side, 6-7 on the edge_i side; four edges stored (later, earlier) with the inverse
    measurement; a second, slightly different edge 2-3; a free pose without any edge at the end (index 14)"""
    rng = np.random.default_rng(14)
    P, _ = chain(rng, 14, drift=0.05)
    const = P.pose_const.copy()
    const[[0, 5, 6, 13]] = 1
    ei, ej, Tij = P.edge_i.copy(), P.edge_j.copy(), P.T_ij.copy()
    for e in (1, 4, 8, 11):
        ei[e], ej[e], Tij[e] = P.edge_j[e], P.edge_i[e], _inv7(P.T_ij[e])
    ei, ej = np.append(ei, 2), np.append(ej, 3)
    Tij = np.vstack([Tij, pose7(mat(P.T_ij[2]) @ expm(hat6(rng.normal(0, 0.02, 6))))])
    for k in np.flatnonzero(const == 0):     # dead reckoning alone converges in two steps: start further off
        P.pose[k] = pose7(mat(P.pose[k]) @ expm(hat6(rng.normal(0, 0.2, 6))))
    pose = np.vstack([P.pose, pose7(expm(hat6(np.array([2.0, -1.0, 0.5, 0.2, 0.3, -0.1]))))])
    return T.PgProblem(pose, np.append(const, 0), ei, ej, Tij)


def with_inserted_constants(P, after=(1, 2, 7, 10)):
    """the same graph with an unrelated constant pose (no edge) put in after each pose of `after`: the index of a free
    pose among the free poses no longer follows from its pose index"""
    new_of_old, pose, const = [], [], []
    for k in range(len(P.pose)):
        new_of_old.append(len(pose))
        pose.append(P.pose[k]); const.append(P.pose_const[k])
        if k in after:
            pose.append(pose7(expm(hat6(np.array([0.1 * k, 1.0, -2.0, 0.3, 0.1 * k, -0.2])))))
            const.append(1)
    m = np.array(new_of_old)
    return T.PgProblem(np.stack(pose), np.array(const, np.uint8), m[P.edge_i], m[P.edge_j], P.T_ij)


def with_scaled_quaternions(P, seed=5):
    """quaternions of poses and measurements scaled to norm 1 +- 1e-3: both sides normalise before use"""
    rng = np.random.default_rng(seed)
    Q = P.copy()
    Q.pose[:, 3:] *= 1.0 + rng.choice([-1e-3, 1e-3], (len(Q.pose), 1))
    Q.T_ij = Q.T_ij.copy()
    Q.T_ij[:, 3:] *= 1.0 + rng.choice([-1e-3, 1e-3], (len(Q.T_ij), 1))
    return Q


def runs(const, seed, noise=0.02, pert=0.05, edges="all"):
    """a chain over the arc whose constant poses (exact) cut it into independent runs of free poses (perturbed by
    `pert`); odometry with noise `noise`; edges "all", or "left": only the edge from the pose before, for every free pose"""
    rng = np.random.default_rng(seed)
    const = np.asarray(const, np.uint8)
    n = len(const)
    step = expm(hat6(np.array([0.5, 0.02, 0.0, 0.0, 0.1, 0.02])))
    gt = [np.eye(4)]
    for k in range(1, n):
        gt.append(gt[-1] @ step)
    noise6 = rng.normal(0, noise, (n - 1, 6))
    pert6 = rng.normal(0, pert, (n, 6))
    est = [gt[k] if const[k] else gt[k] @ expm(hat6(pert6[k])) for k in range(n)]
    keep = [k for k in range(1, n) if not (const[k - 1] and const[k]) and (edges == "all" or not const[k])]
    Tij = [pose7(step @ expm(hat6(noise6[k - 1]))) for k in keep]
    return T.PgProblem(np.stack([pose7(M) for M in est]), const, [k - 1 for k in keep], keep, np.stack(Tij))


def alternating(n, seed, edges="all"):
    """constant / free / constant ...: every free pose a run of its own"""
    return runs(np.arange(n) % 2 == 0, seed, edges=edges)


def mixed_runs(seed=3):
    """runs of 1, 2, 3, 4, 5, 1 and 3 free poses between single constants, the last run open-ended"""
    const = [1]
    for length in (1, 2, 3, 4, 5, 1, 3):
        const += [0] * length + [1]
    return runs(const[:-1], seed)


def _shape_cases():
    S = shapes14()
    o = dict(max_iters=10, function_tolerance=1e-8)
    few = dict(max_iters=3, function_tolerance=1e-8)
    out = [
        Case("shapes14", S, o, dict(min_accepted=3, isolated=14)),
        Case("shapes14_inserted_constants", with_inserted_constants(S), o, dict(min_accepted=3, isolated=18)),
        Case("shapes14_scaled_quaternions", with_scaled_quaternions(S), o, dict(min_accepted=3)),
        Case("mixed_runs", mixed_runs(), o, dict(min_accepted=3)),
    ]
    for n in (511, 513, 514):      # nf = n_seg = 255, 256, 257; n_edge = 510, 512, 513 / 255, 256, 257
        out.append(Case("alternating_%d" % n, alternating(n, n), few, dict(termination=MAX_ITER, flags="AAAA")))
        # one edge per free pose: a zero-residual problem, damped by a unit radius to stay above its rounding floor
        out.append(Case("alternating_%d_left_edges" % n, alternating(n, n, edges="left"), dict(few, initial_radius=1.0),
                        dict(termination=MAX_ITER, flags="AAAA")))
    return out


# ---- the problems tests/test_pg_gpu.py had before these cases (scripts/oracle_cov.py pg_cases:legacy_cases) ------------------

def legacy_cases():
    out = [Case("local_%d" % n, chain(np.random.default_rng(n), n, drift=d)[0], {}, {})
           for n, d in ((8, 0.01), (40, 0.01), (200, 0.003))]
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
    out.append(Case("full_300", T.PgProblem(np.stack([pose7(M) for M in est]), const, np.arange(n - 1), np.arange(1, n),
                                            np.stack(meas)), dict(max_iters=100, function_tolerance=1e-6), {}))
    out.append(Case("consistent", chain(np.random.default_rng(2), 12, drift=0.01, loop=False)[0], {}, {}))
    Q, _ = chain(np.random.default_rng(2), 6)
    Q.pose_const[:] = 1
    out.append(Case("all_constant", Q, {}, {}))
    S, _ = chain(np.random.default_rng(4), 20)
    S.pose_const[10] = 1
    out.append(Case("split", S, {}, {}))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _wild_cases() + _log_cases() + _shape_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def ids():
    return [c.name for c in cases()]
