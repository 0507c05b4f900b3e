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
        r["stats"] = dict(zip(_LOOP_STATS, st.tolist()))
        return r

    def set_close(self, on):
        """LoopCloser::close_loops_: new_keyframe goes on to closeLoop on an accepted loop (off by default)"""
        self.L.ov2h_loop_closer_set_close.argtypes = [vp, C.c_int]
        self.L.ov2h_loop_closer_set_close(self.h, int(bool(on)))

    def closed(self, cap=1 << 14):
        """`closed` of the last new_keyframe result (host_map.unpack_close layout; an untouched result when nothing was closed)"""
        from .host_map import unpack_close
        ints, dbl, merged, st = np.zeros(9, np.int32), np.zeros(3), np.zeros(cap, np.int32), np.zeros(3, np.int32)
        self.L.ov2h_loop_closer_closed.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        rc = self.L.ov2h_loop_closer_closed(self.h, cap, ints.ctypes.data_as(vp), dbl.ctypes.data_as(vp), merged.ctypes.data_as(vp),
                                            st.ctypes.data_as(vp))
        if rc != 0:
            raise RuntimeError(f"ov2h_loop_closer_closed: status {rc}")
        return unpack_close(ints, dbl, merged, st)

    def set_brief_pattern(self, pattern):
        """the 256 BRIEF-32 test pairs (256 x {y1, x1, y2, x2}, int8) the extra keypoints are described with"""
        pat = np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
        self.L.ov2h_loop_set_brief_pattern.argtypes = [vp, vp]
        self.L.ov2h_loop_set_brief_pattern(self.h, pat.ctypes.data_as(vp))

    def set_extra_cap(self, cap):
        """room per image of the first detect call of extraKeypoints"""
        self.L.ov2h_loop_set_extra_cap.argtypes = [vp, C.c_int]
        self.L.ov2h_loop_set_extra_cap(self.h, int(cap))

    def detector_counts(self):
        """Detector.counts() of the closer's own detector (None before its first keyframe)"""
        self.L.ov2h_loop_closer_detector.restype = vp
        self.L.ov2h_loop_closer_detector.argtypes = [vp]
        h = self.L.ov2h_loop_closer_detector(self.h)
        if not h:
            return None
        out = np.zeros(10, np.int32)
        self.L.ov2h_lcd_counts(vp(h), out.ctypes.data_as(vp))
        return dict(zip(("images", "words", "dev_slots", "dev_live", "dev_compactions", "n_add_matches", "n_matches", "n_added",
                         "n_purged", "n_islands"), out.tolist()))

    def new_keyframe_img(self, kfid, seed, pyr, b=0):
        """newKeyframe with the keyframe's raw image (image b of `pyr`): the extra FAST + BRIEF keypoints go to the detector too"""
        return new_keyframes([self], [kfid], [seed], pyr, [b])[0]


_LOOP_STATS = ("pairs", "knn_pairs", "epi_pairs", "knn_calls", "epi_calls", "p3p_pairs", "refine_pairs", "track_pairs", "pnp_pairs",
               "p3p_calls", "refine_calls", "track_calls", "pnp_calls")


def _closer_args(closers, kfids, bs):
    B = len(closers)
    return (B, (vp * B)(*[c.h for c in closers]), np.ascontiguousarray(kfids, np.int32), np.ascontiguousarray(bs, np.int32))


def extra_keypoints(closers, kfids, pyr, bs, cap=4096):
    """LoopCloser::extraKeypoints for B closers: one dict per job (skipped, nbkps, mask_xy, n_detected, add_xy, add_resp, add_desc)
    and the (detect, describe) call counts"""
    L = closers[0].L
    B, hs, kf, b = _closer_args(closers, kfids, bs)
    counts, stats = np.zeros((B, 5), np.int32), np.zeros(2, np.int32)
    mxy, axy = np.zeros((B, cap, 2), np.float32), np.zeros((B, cap, 2), np.float32)
    ar, ad = np.zeros((B, cap), np.uint8), np.zeros((B, cap, 32), np.uint8)
    P = lambda a: a.ctypes.data_as(vp)
    L.ov2h_loop_extra_keypoints.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    rc = L.ov2h_loop_extra_keypoints(B, hs, P(kf), pyr.h, P(b), cap, P(counts), P(mxy), P(axy), P(ar), P(ad), P(stats))
    if rc != 0:
        raise RuntimeError(f"extraKeypoints: status {rc}")
    jobs = [dict(skipped=int(c[0]), nbkps=int(c[1]), mask_xy=mxy[k, :c[2]].copy(), n_detected=int(c[3]), add_xy=axy[k, :c[4]].copy(),
                 add_resp=ar[k, :c[4]].copy(), add_desc=ad[k, :c[4]].copy()) for k, c in enumerate(counts)]
    return jobs, dict(detect_calls=int(stats[0]), describe_calls=int(stats[1]))


def new_keyframes(closers, kfids, seeds, pyr, bs):
    """LoopCloser::newKeyframes: B closers stepped together on the images bs of `pyr`; one dict per closer as new_keyframe returns
    it, plus nbkps, n_extra, n_descs and `extra` = the (detect, describe) call counts of the step"""
    L = closers[0].L
    B, hs, kf, b = _closer_args(closers, kfids, bs)
    sd = np.ascontiguousarray(seeds, np.uint64)
    out, st, es = np.zeros((B, 13), np.int32), np.zeros((B, 13), np.int32), np.zeros(2, np.int32)
    P = lambda a: a.ctypes.data_as(vp)
    L.ov2h_loop_new_keyframes_img.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    rc = L.ov2h_loop_new_keyframes_img(B, hs, P(kf), P(sd), pyr.h, P(b), P(out), P(st), P(es))
    if rc != 0:
        raise RuntimeError(f"newKeyframes: status {rc}")
    res = []
    for k in range(B):
        r = dict(zip(("skipped", "image_id", "status", "train_id", "cand_kfid", "lckfid", "branch", "n_passed", "verify_branch", "n_final",
                      "nbkps", "n_extra", "n_descs"), out[k].tolist()))
        r["stats"] = dict(zip(_LOOP_STATS, st[k].tolist()))
        r["extra"] = dict(detect_calls=int(es[0]), describe_calls=int(es[1]))
        res.append(r)
    return res
