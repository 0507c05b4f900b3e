"""numpy checker for the graph Optimizer::assembleLocalPoseGraph builds (reference src/optimizer.cpp:2361-2425): the chain
rules on a set of live keyframe ids, and the edge measurements as 4 x 4 products.  Shares nothing with the C++ host stage or
the kernel (csrc/map.hip, mp_assemble_kernel) but the statement it restates."""
import numpy as np

from loop_close_ref import mat


def chain(alive, newkf, kfloop_id):
    """alive: the ids of the live keyframes.  Returns the listed ids -- the loop keyframe after the walk-up, then the live
    keyframes up to newkf, ascending -- or None: a dead newkf, no live loop keyframe below it, fewer than two poses."""
    alive = set(int(k) for k in alive)
    if newkf not in alive:
        return None
    top = max(alive)
    k = int(kfloop_id)
    while k not in alive and k < top:          # :2368-2371
        k += 1
    if k not in alive:
        return None
    ids = [k] + [q for q in range(k + 1, newkf + 1) if q in alive]     # :2389-2420
    if len(ids) < 2 or ids[-1] != newkf:
        return None
    return ids


def assemble(poses, alive, newkf, kfloop_id, newTwc):
    """poses: {kfid: 7-vector}.  Returns None or dict(kfids, pose (n x 7, the stored vectors), pose_const, edge_i, edge_j,
    T_ij: list of n 4 x 4 matrices, inverse(Twc_i) @ Twc_j for the n - 1 odometry edges, then inverse(Twc_loop) @ newTwc for
    the closing edge (0, n - 1))"""
    ids = chain(alive, newkf, kfloop_id)
    if ids is None:
        return None
    n = len(ids)
    M = [mat(poses[k]) for k in ids]
    T = [np.linalg.inv(M[i]) @ M[i + 1] for i in range(n - 1)] + [np.linalg.inv(M[0]) @ mat(newTwc)]
    return dict(kfids=np.array(ids, np.int32), pose=np.stack([np.asarray(poses[k], np.float64) for k in ids]),
                pose_const=np.array([1] + [0] * (n - 1), np.uint8), edge_i=np.array(list(range(n - 1)) + [0], np.int32),
                edge_j=np.array(list(range(1, n)) + [n - 1], np.int32), T_ij=T)
