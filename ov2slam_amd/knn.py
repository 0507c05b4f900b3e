"""ctypes binding of the loop-candidate matcher (ov2_knn2_hamming_batch, include/ov2slam_hip.h): the two nearest train
descriptors of every query descriptor by Hamming distance, B pairs per call.  Plumbing only; the arithmetic is the kernel's."""
import ctypes as C

import numpy as np

from .frontend import _check

MAX_TRAIN, MAX_ROWS, MAX_BATCH, TILE = 65536, 1 << 24, 65535, 1024   # OV2_KNN_* of the header


def _flat(blocks):
    rows = [np.ascontiguousarray(b, np.uint8).reshape(-1, 32) for b in blocks]
    n = np.array([len(r) for r in rows], np.int32)
    return n, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8))


def knn2_hamming_batch(ctx, queries, trains):
    """queries / trains: B arrays of n x 32 uint8 each.  Returns per pair (idx (n_query, 2) int32, dist (n_query, 2) int32)."""
    nq, q = _flat(queries)
    nt, t = _flat(trains)
    assert len(nq) == len(nt)
    idx, dist = np.full((len(q), 2), -7, np.int32), np.full((len(q), 2), -7, np.int32)
    vp = C.c_void_p
    _check(ctx.h, ctx.lib.ov2_knn2_hamming_batch(ctx.h, len(nq), nq.ctypes.data_as(vp), nt.ctypes.data_as(vp), q.ctypes.data_as(vp),
                                                 t.ctypes.data_as(vp), idx.ctypes.data_as(vp), dist.ctypes.data_as(vp)))
    o = np.concatenate([[0], np.cumsum(nq)])
    return [(idx[o[b]:o[b + 1]], dist[o[b]:o[b + 1]]) for b in range(len(nq))]


def knn2_hamming_batch_dev(ctx, queries, trains, fill=-7):
    """the device-resident form on arrays uploaded here; idx / dist start as `fill` so that untouched slots show.  Returns the
    flat (idx, dist) of all query rows, each (sum(n_query), 2)."""
    nq, q = _flat(queries)
    nt, t = _flat(trains)
    qo = np.concatenate([[0], np.cumsum(nq)]).astype(np.int32)
    to = np.concatenate([[0], np.cumsum(nt)]).astype(np.int32)
    d_qo, d_to, d_q, d_t = ctx.to_device(qo), ctx.to_device(to), ctx.to_device(q), ctx.to_device(t)
    d_idx = ctx.to_device(np.full((len(q), 2), fill, np.int32))
    d_dist = ctx.to_device(np.full((len(q), 2), fill, np.int32))
    _check(ctx.h, ctx.lib.ov2_knn2_hamming_batch_dev(ctx.h, len(nq), len(q), d_qo.ptr, d_to.ptr, d_q.ptr, d_t.ptr, d_idx.ptr, d_dist.ptr))
    ctx.synchronize()
    return d_idx.get(), d_dist.get()
