"""Host-side mirror of the Ceres problems of Optimizer::localPoseGraph / fullPoseGraph (reference
src/optimizer.cpp:2346-2592, 2783-2870) over the C ABI: a PgProblem (ba_types.py) goes to ov2_pose_graph_solve, which runs
the whole LM loop on the MI355X.  Plumbing only."""
import ctypes as C

from . import _lib
from .ba_types import BaOptionsC, PgProblemC, PgResultC, dp
from .frontend import _check


def default_options(max_iters=10, function_tolerance=1e-4):
    """options.max_num_iterations / function_tolerance of localPoseGraph (:2445-2446) on the Ceres trust-region defaults;
    fullPoseGraph: 100, 1e-6 (:2821-2824)"""
    o = BaOptionsC()
    _lib.load().ov2_ba_default_options(C.byref(o), 5.9915)
    o.max_iters, o.function_tolerance = max_iters, function_tolerance
    return o


def solve(ctx, problem, options=None):
    """solves `problem` (PgProblem) in place; returns PgResultC (costs, termination, iteration log)"""
    o = options if options is not None else default_options()
    res = PgResultC()
    pc = problem.as_c()
    _check(ctx.h, ctx.lib.ov2_pose_graph_solve(ctx.h, C.byref(pc), C.byref(o), C.byref(res)))
    return res


def solve_batch(ctx, problems, options=None):
    """ov2_pose_graph_solve_batch: every PgProblem of `problems` solved in place by one launch (one workgroup per graph),
    each bit-identical to solve() on it; returns the list of PgResultC.  A graph the single call would refuse refuses the
    whole call and leaves every pose array as it was."""
    o = options if options is not None else default_options()
    B = len(problems)
    pcs = (PgProblemC * max(B, 1))(*[p.as_c() for p in problems])
    rcs = (PgResultC * max(B, 1))()
    _check(ctx.h, ctx.lib.ov2_pose_graph_solve_batch(ctx.h, B, pcs, C.byref(o), rcs))
    return [PgResultC.from_buffer_copy(rcs[k]) for k in range(B)]


def _addr(a):
    """the device address behind an int, a DeviceArray (.ptr) or a torch tensor (.data_ptr())"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    p = getattr(a, "ptr", a)
    return getattr(p, "value", p)


def solve_batch_dev(ctx, problems, d_pose, d_T_ij, d_results, options=None):
    """ov2_pose_graph_solve_batch_dev: the structure (sizes, pose_const, edge_i, edge_j) of every PgProblem of `problems` comes
    from the host; d_pose[b] / d_T_ij[b] are the device arrays (n_pose x 7, n_edge x 7 float64: int address, DeviceArray or
    torch tensor) the graph is solved in, d_results the device array of len(problems) ov2_pg_result records
    (ctypes.sizeof(PgResultC) bytes each).  Enqueues and returns: nothing is read back, nothing synchronises."""
    o = options if options is not None else default_options()
    B = len(problems)
    assert len(d_pose) == len(d_T_ij) == B
    pcs = (PgProblemC * max(B, 1))()
    for b, p in enumerate(problems):
        pc = p.as_c()
        pc.pose, pc.T_ij = C.cast(C.c_void_p(_addr(d_pose[b])), dp), C.cast(C.c_void_p(_addr(d_T_ij[b])), dp)
        pcs[b] = pc
    _check(ctx.h, ctx.lib.ov2_pose_graph_solve_batch_dev(ctx.h, B, pcs, C.byref(o), C.c_void_p(_addr(d_results))))
