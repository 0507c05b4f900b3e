"""ctypes binding of the loop detector's device word table and its exact search (ov2_lcd_table_*, ov2_lcd_search2_batch,
include/ov2slam_hip.h) and of the host detector (ov2h_lcd_*, ov2slam_amd/host/ov2_lcd.hpp).  Plumbing only; the arithmetic
is the kernel's and the host library's."""
import ctypes as C

import numpy as np

from .frontend import _check

MAX_WORDS, MAX_BATCH, MAX_QUERY, MAX_SPLITS, TILE = 1 << 22, 4096, 1 << 20, 1024, 512   # OV2_LCD_* of the header
vp = C.c_void_p


def _rows(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 32)


def set_splits(ctx, splits):
    """ov2_lcd_set_splits: 0 = by call size, otherwise the forced number of train-axis splits"""
    _check(ctx.h, ctx.lib.ov2_lcd_set_splits(ctx.h, int(splits)))


def search_calls(ctx):
    n = C.c_longlong()
    _check(ctx.h, ctx.lib.ov2_lcd_search_calls(ctx.h, C.byref(n)))
    return n.value


class Table:
    """one index's live descriptors in HBM"""

    def __init__(self, ctx, capacity_hint=0):
        self.ctx, self.h = ctx, vp()
        _check(ctx.h, ctx.lib.ov2_lcd_table_create(ctx.h, int(capacity_hint), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.ov2_lcd_table_destroy(self.h)
            self.h = None

    __del__ = close

    def append(self, descs):
        d = _rows(descs)
        first = C.c_int()
        _check(self.ctx.h, self.ctx.lib.ov2_lcd_table_append(self.ctx.h, self.h, len(d), d.ctypes.data_as(vp), C.byref(first)))
        return first.value

    def kill(self, slots):
        s = np.ascontiguousarray(slots, np.int32)
        _check(self.ctx.h, self.ctx.lib.ov2_lcd_table_kill(self.ctx.h, self.h, len(s), s.ctypes.data_as(vp)))

    def compact(self):
        _check(self.ctx.h, self.ctx.lib.ov2_lcd_table_compact(self.ctx.h, self.h))

    def count(self):
        """(slots, live, compactions)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.h, self.ctx.lib.ov2_lcd_table_count(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ids(self):
        """(word id of every slot, dead flag of every slot)"""
        n = self.count()[0]
        ids, dead = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        _check(self.ctx.h, self.ctx.lib.ov2_lcd_table_ids(self.h, n, ids.ctypes.data_as(vp), dead.ctypes.data_as(vp)))
        return ids, dead.astype(bool)


def _flat(queries):
    rows = [_rows(q) for q in queries]
    n = np.array([len(r) for r in rows], np.int32)
    return n, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8))


def _handles(tables):
    return (vp * max(len(tables), 1))(*[t.h for t in tables])


def _split(nq, idx, dist):
    o = np.concatenate([[0], np.cumsum(nq)])
    return [(idx[o[b]:o[b + 1]], dist[o[b]:o[b + 1]]) for b in range(len(nq))]


def search2_batch(ctx, tables, queries, fill=-7):
    """tables: B Table objects, queries: B arrays of n x 32 uint8.  Returns per pair (idx (n, 2), dist (n, 2)) int32."""
    nq, q = _flat(queries)
    assert len(nq) == len(tables)
    idx, dist = np.full((len(q), 2), fill, np.int32), np.full((len(q), 2), fill, np.int32)
    _check(ctx.h, ctx.lib.ov2_lcd_search2_batch(ctx.h, len(nq), _handles(tables), nq.ctypes.data_as(vp), q.ctypes.data_as(vp),
                                                idx.ctypes.data_as(vp), dist.ctypes.data_as(vp)))
    return _split(nq, idx, dist)


def search2_batch_dev(ctx, tables, queries, fill=-7, extra_rows=0):
    """the device-resident form on arrays uploaded here; idx / dist have extra_rows rows more than the call writes and start
    as `fill`, so that untouched slots show.  Returns the flat (idx, dist)."""
    nq, q = _flat(queries)
    d_q = ctx.to_device(q if len(q) else np.zeros((1, 32), np.uint8))
    d_idx = ctx.to_device(np.full((len(q) + extra_rows, 2), fill, np.int32))
    d_dist = ctx.to_device(np.full((len(q) + extra_rows, 2), fill, np.int32))
    _check(ctx.h, ctx.lib.ov2_lcd_search2_batch_dev(ctx.h, len(nq), _handles(tables), nq.ctypes.data_as(vp), d_q.ptr, d_idx.ptr, d_dist.ptr))
    ctx.synchronize()
    return d_idx.get(), d_dist.get()


# ---- host detector (libov2host.so) ------------------------------------------------------------------------------------------

_host = None


def host_lib():
    global _host
    if _host is None:
        import os
        L = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libov2host.so"))
        L.ov2h_lcd_create.restype = vp
        L.ov2h_lcd_create.argtypes = [vp, C.c_int, C.c_float, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ov2h_lcd_destroy.argtypes = [vp]
        L.ov2h_lcd_process_batch.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
        L.ov2h_lcd_counts.argtypes = [vp, vp]
        L.ov2h_lcd_trace.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]
        _host = L
    return _host


class Detector:
    """ov2::LCDetector.  ctx = None: the host brute-force back end; otherwise the device word table on that context."""

    def __init__(self, ctx=None, p=100, nndr=0.8, min_score=0.3, island_size=20, nframes_after_lc=10, purge_descriptors=True,
                 min_feat_apps=2):
        self.L, self.ctx = host_lib(), ctx
        self.h = vp(self.L.ov2h_lcd_create(ctx.h if ctx is not None else None, p, nndr, min_score, island_size, nframes_after_lc,
                                           int(purge_descriptors), min_feat_apps))

    def close(self):
        if getattr(self, "h", None):
            self.L.ov2h_lcd_destroy(self.h)
            self.h = None

    __del__ = close

    def process(self, image_id, descs):
        return process_batch([self], [image_id], [descs])[0]

    def counts(self):
        out = np.zeros(10, np.int32)
        self.L.ov2h_lcd_counts(self.h, out.ctypes.data_as(vp))
        return dict(zip(("images", "words", "dev_slots", "dev_live", "dev_compactions", "n_add_matches", "n_matches", "n_added",
                         "n_purged", "n_islands"), out.tolist()))

    def trace(self):
        """the last process call: dict(add_matches, matches [(query row, word id, distance)], added, purged, scores, islands
        [(img_id, min, max, score)])"""
        c = self.counts()
        am, m = np.zeros((c["n_add_matches"], 3), np.int32), np.zeros((c["n_matches"], 3), np.int32)
        ad, pu = np.zeros(c["n_added"], np.int32), np.zeros(c["n_purged"], np.int32)
        sc, isl, isc = np.zeros(c["images"], np.float64), np.zeros((c["n_islands"], 3), np.int32), np.zeros(c["n_islands"], np.float64)
        P = lambda a: a.ctypes.data_as(vp)
        ns = self.L.ov2h_lcd_trace(self.h, P(am), P(m), P(ad), P(pu), P(sc), len(sc), P(isl), P(isc))
        return dict(add_matches=[tuple(r) for r in am.tolist()], matches=[tuple(r) for r in m.tolist()], added=ad.tolist(),
                    purged=pu.tolist(), scores=sc[:ns].tolist(), islands=[(*r, s) for r, s in zip(isl.tolist(), isc.tolist())])


def process_batch(dets, image_ids, descs):
    """LCDetector::processBatch over B detectors of one back end.  Returns [(status, train_id)]."""
    B = len(dets)
    rows = [_rows(d) for d in descs]
    hs = (vp * B)(*[d.h for d in dets])
    ids = np.asarray(image_ids, np.uint32)
    ptrs = (vp * B)(*[r.ctypes.data_as(vp) for r in rows])
    n = np.array([len(r) for r in rows], np.int32)
    st, tr = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = dets[0].L.ov2h_lcd_process_batch(B, hs, ids.ctypes.data_as(vp), ptrs, n.ctypes.data_as(vp), st.ctypes.data_as(vp), tr.ctypes.data_as(vp))
    if rc != 0:
        ctx = dets[0].ctx
        _check(ctx.h if ctx is not None else None, rc)
    return list(zip(st.tolist(), tr.tolist()))


class LoopCloser:
    """ov2::LoopCloser that lives across keyframes, on a host_map.LoopMap: newKeyframe = the body of LoopCloser::run for one
    keyframe (detector, candidate, processLoopCandidates)"""

    def __init__(self, ctx, loop_map, p=100, nndr=0.8, min_score=0.3, island_size=20, nframes_after_lc=10, purge_descriptors=True,
                 min_feat_apps=2, nransac_iter=100, fransac_err=3.0):
        L = host_lib()
        L.ov2h_loop_closer_create.restype = vp
        L.ov2h_loop_closer_create.argtypes = [vp, vp, C.c_int, C.c_float, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
        L.ov2h_loop_closer_destroy.argtypes = [vp]
        L.ov2h_loop_new_keyframe.argtypes = [vp, C.c_int, C.c_ulonglong, vp, vp]
        self.L, self.map = L, loop_map   # the map must outlive the closer
        self.h = vp(L.ov2h_loop_closer_create(loop_map.h, ctx.h, p, nndr, min_score, island_size, nframes_after_lc, int(purge_descriptors),
                                              min_feat_apps, nransac_iter, fransac_err))

    def close(self):
        if getattr(self, "h", None):
            self.L.ov2h_loop_closer_destroy(self.h)
            self.h = None

    __del__ = close

    def new_keyframe(self, kfid, seed):
        out, st = np.zeros(10, np.int32), np.zeros(13, np.int32)
        rc = self.L.ov2h_loop_new_keyframe(self.h, int(kfid), int(seed), out.ctypes.data_as(vp), st.ctypes.data_as(vp))
        if rc != 0:
            raise RuntimeError(f"newKeyframe: status {rc}")
        r = dict(zip(("skipped", "image_id", "status", "train_id", "cand_kfid", "lckfid", "branch", "n_passed", "verify_branch", "n_final"),
                     out.tolist()))
        r["stats"] = dict(zip(("pairs", "knn_pairs", "epi_pairs", "knn_calls", "epi_calls", "p3p_pairs", "refine_pairs", "track_pairs",
                               "pnp_pairs", "p3p_calls", "refine_calls", "track_calls", "pnp_calls"), st.tolist()))
        return r
