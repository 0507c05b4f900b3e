"""Host-side mirror of the keyframe descriptor path over the C ABI (first half):
  describeBRIEF  <- FeatureExtractor::describeBRIEF  src/feature_extractor.cpp:224-285
  matchToMap     <- Mapper::matchToMap               src/mapper.cpp:576-774 (flat inputs: MatchInput)
  matchToMap_batch(_dev) <- the same for B frames, one local map each, in one call (flat inputs: MatchBatchInput)
Plumbing only (ctypes + numpy); the box sums, projections and Hamming distances run in csrc/match.hip."""
import ctypes as C

import numpy as np

from .frontend import _check

f32p, f64p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


class MatchInputC(C.Structure):
    _fields_ = [("Twc", C.c_double * 7), ("K", C.c_double * 4), ("img_w", C.c_int32), ("img_h", C.c_int32), ("cell", C.c_int32),
                ("nb3dkps", C.c_int32), ("n_kp", C.c_int32), ("kp_px", f32p), ("kp_desc_ptr", i32p), ("kp_descs", u8p),
                ("kp_kf_ptr", i32p), ("kp_kfids", i32p), ("kp_kf_px", f32p), ("grid_ptr", i32p), ("grid_kp", i32p),
                ("n_cand", C.c_int32), ("cand_wpt", f64p), ("cand_desc_ptr", i32p), ("cand_descs", u8p), ("cand_kf_ptr", i32p),
                ("cand_kfids", i32p), ("n_kf", C.c_int32), ("kf_Twc", f64p), ("cam", C.c_void_p)]


class MatchBatchInputC(C.Structure):
    _fields_ = [("B", C.c_int32), ("n_kp", C.c_int32), ("n_cand", C.c_int32), ("K", C.c_double * 4), ("img_w", C.c_int32),
                ("img_h", C.c_int32), ("cell", C.c_int32), ("cam", C.c_void_p), ("Twc", f64p), ("nb3dkps", i32p), ("kp_off", i32p),
                ("cand_off", i32p), ("kf_off", i32p), ("kp_px", f32p), ("kp_desc_ptr", i32p), ("kp_descs", u8p), ("kp_kf_ptr", i32p),
                ("kp_kfids", i32p), ("kp_kf_px", f32p), ("grid_ptr", i32p), ("grid_kp", i32p), ("cand_wpt", f64p),
                ("cand_desc_ptr", i32p), ("cand_descs", u8p), ("cand_kf_ptr", i32p), ("cand_kfids", i32p), ("kf_Twc", f64p)]


def _arrays(struct):
    """the array fields of a matcher's C struct, in its order: (name, pointer type)"""
    return tuple((name, t) for name, t in struct._fields_ if t in (f32p, f64p, i32p, u8p))


BATCH_ARRAYS = _arrays(MatchBatchInputC)
MATCH_BATCH_WAVES = 4   # candidates per workgroup of match_cand_kernel (csrc/match.hip); the results do not depend on it


def _csr(lists, dtype, width=1):
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype).reshape(-1, width) for x in lists]) if len(lists) and ptr[-1] else np.zeros((0, width), dtype)
    return ptr, np.ascontiguousarray(flat.reshape(-1, width) if width > 1 else flat.ravel(), dtype)


class _MatcherInput:
    """what the inputs of the three matchers share: the keypoint and candidate arrays of `frames` (a list of dicts with kps and
    cands; the loop closer's pairs are such frames) back to back, each frame's grid (Frame::vgridkps_, rebuilt from its kp
    order = insertion order), the offsets, and the fill of the C struct."""

    def _build(self, frames, img_w, img_h, cell):
        """sets the shared arrays; returns the keypoints of all frames in order, for the arrays only one matcher has"""
        c = np.ascontiguousarray
        kps = [k for f in frames for k in f["kps"]]
        cands = [q for f in frames for q in f["cands"]]
        self.kp_off, self.cand_off = self._off(frames, "kps"), self._off(frames, "cands")
        self.kp_px = c([k["px"] for k in kps], np.float32).reshape(-1, 2)
        self.kp_desc_ptr, self.kp_descs = _csr([k["descs"] for k in kps], np.uint8, 32)
        self.kp_kf_ptr, self.kp_kfids = _csr([k["kfids"] for k in kps], np.int32)
        nbw, nbh = int(np.ceil(np.float32(img_w) / np.float32(cell))), int(np.ceil(np.float32(img_h) / np.float32(cell)))
        self.ncells = nbw * nbh
        cells = [[] for _ in range(len(frames) * self.ncells)]
        for b, f in enumerate(frames):
            for i, k in enumerate(f["kps"]):
                r = int(np.floor(np.float32(k["px"][1]) / np.float32(cell)))
                cc = int(np.floor(np.float32(k["px"][0]) / np.float32(cell)))
                cells[b * self.ncells + r * nbw + cc].append(i)
        self.grid_ptr, self.grid_kp = _csr(cells, np.int32)
        self.cand_wpt = c([q["wpt"] for q in cands], np.float64).reshape(-1, 3)
        self.cand_desc_ptr, self.cand_descs = _csr([q["descs"] for q in cands], np.uint8, 32)
        self.cand_kf_ptr, self.cand_kfids = _csr([q["kfids"] for q in cands], np.int32)
        return kps

    @staticmethod
    def _off(frames, key):
        return np.concatenate([[0], np.cumsum([len(f[key]) for f in frames])]).astype(np.int32)

    def _fill(self, m, K, img_w, img_h, cell, cam):
        """the counts, the camera and every array of self into the C struct m, which becomes self.c"""
        self.cam = cam   # None or ba_types.CamModelC
        m.n_kp, m.n_cand = len(self.kp_px), len(self.cand_wpt)
        m.K[:] = np.asarray(K, np.float64).tolist()
        m.img_w, m.img_h, m.cell = int(img_w), int(img_h), int(cell)
        m.cam = None if cam is None else C.addressof(cam)
        for name, t in _arrays(type(m)):
            setattr(m, name, getattr(self, name).ctypes.data_as(t))
        self.c = m


class MatchInput(_MatcherInput):
    """owns the flat arrays of one Mapper::matchToMap call.
    kps: list of dict(px (2,), descs (d,32) u8, kfids [ascending], kf_px (len(kfids),2)); cands: list of dict(wpt (3,), descs,
    kfids); kf_Twc: (n_kf, 7) indexed by kfid; the grid (Frame::vgridkps_) is rebuilt from kp order = insertion order.
    cam: None or ba_types.CamModelC, the lens model of the projections."""

    def __init__(self, Twc, K, img_w, img_h, cell, nb3dkps, kps, cands, kf_Twc, cam=None):
        self._build([dict(kps=kps, cands=cands)], img_w, img_h, cell)
        _, self.kp_kf_px = _csr([k["kf_px"] for k in kps], np.float32, 2)
        self.kf_Twc = np.ascontiguousarray(kf_Twc, np.float64).reshape(-1, 7)
        m = MatchInputC()
        m.Twc[:] = np.asarray(Twc, np.float64).tolist()
        m.nb3dkps, m.n_kf = int(nb3dkps), len(self.kf_Twc)
        self._fill(m, K, img_w, img_h, cell, cam)


class MatchBatchInput(_MatcherInput):
    """owns the flat arrays of one ov2_match_to_map_batch call.
    frames: list of dict(Twc (7,), kps, cands, kf_Twc (n_kf, 7)) with kps / cands as MatchInput takes them; nb3dkps: one count
    per frame (Frame::nb3dkps_: under 30 the pixel gate of that frame doubles).  Each frame's grid (Frame::vgridkps_) is rebuilt
    from its kp order = insertion order.  cam: None or ba_types.CamModelC (one camera per call)."""

    def __init__(self, frames, K, img_w, img_h, cell, nb3dkps, cam=None):
        c, B = np.ascontiguousarray, len(frames)
        kps = self._build(frames, img_w, img_h, cell)
        self.Twc = c([f["Twc"] for f in frames], np.float64).reshape(-1, 7)
        self.nb3dkps = c(np.broadcast_to(np.asarray(nb3dkps, np.int32), (B,)))
        self.kf_off = self._off(frames, "kf_Twc")
        _, self.kp_kf_px = _csr([k["kf_px"] for k in kps], np.float32, 2)
        self.kf_Twc = c(np.concatenate([np.asarray(f["kf_Twc"], np.float64).reshape(-1, 7) for f in frames]) if B else np.zeros((0, 7)))
        m = MatchBatchInputC()
        m.B = B
        self._fill(m, K, img_w, img_h, cell, cam)

    def split(self, mc, md):
        """the per-frame slices of a call's outputs"""
        o = self.kp_off
        return [(mc[o[b]:o[b + 1]], md[o[b]:o[b + 1]]) for b in range(len(o) - 1)]


def _host_call(ctx, entry, inp, fmaxprojerr, fdistratio):
    """a host-pointer matcher entry point on inp; the outputs start as -7 so that untouched slots show"""
    n = inp.c.n_kp
    mc, md = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.float32)
    _check(ctx.h, getattr(ctx.lib, entry)(ctx.h, C.addressof(inp.c), float(fmaxprojerr), float(fdistratio), mc.ctypes.data, md.ctypes.data))
    return mc[:n], md[:n]


class _MatcherInputDev:
    """a batch input resident in HBM, with the work and output arrays of its _dev entry point ENTRY; the outputs start as
    `fill` so that untouched slots show"""

    def __init__(self, ctx, inp, fill=-7):
        self.ctx, self.host, n = ctx, inp, inp.c.n_kp
        arrays = _arrays(type(inp.c))
        self.dev = {name: ctx.to_device(getattr(inp, name)) for name, _ in arrays}
        self.c = type(inp.c)()
        C.memmove(C.addressof(self.c), C.addressof(inp.c), C.sizeof(self.c))
        for name, t in arrays:
            setattr(self.c, name, C.cast(self.dev[name].ptr, t))
        self.d_work = ctx.to_device(np.zeros(max(n, 1), np.uint64))
        self.d_mc, self.d_md = ctx.to_device(np.full(max(n, 1), fill, np.int32)), ctx.to_device(np.full(max(n, 1), fill, np.float32))

    def enqueue(self, fmaxprojerr=None, fdistratio=0.2):
        """asynchronous: nothing is synchronised.  fmaxprojerr: None = the matcher's default FMAXPROJERR"""
        fmaxprojerr = self.FMAXPROJERR if fmaxprojerr is None else fmaxprojerr
        _check(self.ctx.h, getattr(self.ctx.lib, self.ENTRY)(self.ctx.h, C.addressof(self.c), float(fmaxprojerr), float(fdistratio),
                                                             self.d_work.ptr, self.d_mc.ptr, self.d_md.ptr))

    def get(self):
        n = self.host.c.n_kp
        self.ctx.synchronize()
        return self.d_mc.get()[:n], self.d_md.get()[:n]


def describeBRIEF(ctx, pyr, pts, pattern, b=0):
    """returns (desc (n,32) u8, valid (n,) bool)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    pat = np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
    n = len(pts)
    desc, valid = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    _check(ctx.h, ctx.lib.ov2_describe_brief(ctx.h, pyr.h, int(b), n, pts.ctypes.data, pat.ctypes.data, desc.ctypes.data, valid.ctypes.data))
    return desc, valid.astype(bool)


def matchToMap(ctx, inp, fmaxprojerr=2.0, fdistratio=0.2):
    """returns (match_cand (n_kp,) int32: candidate index or -1, match_dist (n_kp,) f32)"""
    return _host_call(ctx, "ov2_match_to_map", inp, fmaxprojerr, fdistratio)


def matchToMap_batch(ctx, inp, fmaxprojerr=2.0, fdistratio=0.2):
    """host form.  returns (match_cand (n_kp,) int32: candidate index within the frame or -1, match_dist (n_kp,) f32); slice them
    with inp.split"""
    return _host_call(ctx, "ov2_match_to_map_batch", inp, fmaxprojerr, fdistratio)


class MatchBatchInputDev(_MatcherInputDev):
    """a MatchBatchInput resident in HBM, for ov2_match_to_map_batch_dev"""
    ENTRY, FMAXPROJERR = "ov2_match_to_map_batch_dev", 2.0

    def pairs(self, kp_lmid, cand_lmid):
        """ov2_match_pairs_dev behind enqueue(): the matches as the ordered (prevlmid, newlmid) lists of Mapper::mergeMatches,
        one segment per frame (kp_off), ascending prevlmid, -1 behind the pairs.  kp_lmid (n_kp) / cand_lmid (n_cand): the
        lmids of the keypoints and of the candidates, host arrays or DeviceArrays.  Asynchronous; returns the
        device_map.DevPairs that device_map.merge_points_batch(..., dev=True) takes"""
        from .device_map import DevPairs
        ctx, n = self.ctx, self.host.c.n_kp
        up = lambda a: a if hasattr(a, "ptr") else ctx.to_device(np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32))
        d_kl, d_cl = up(kp_lmid), up(cand_lmid)
        d_prev, d_new = ctx.empty(max(n, 1), np.int32), ctx.empty(max(n, 1), np.int32)
        d_np = ctx.empty(max(self.host.c.B, 1), np.int32)
        _check(ctx.h, ctx.lib.ov2_match_pairs_dev(ctx.h, self.host.c.B, n, self.dev["kp_off"].ptr, self.dev["cand_off"].ptr, d_kl.ptr,
                                                  d_cl.ptr, self.d_mc.ptr, d_prev.ptr, d_new.ptr, d_np.ptr))
        out = DevPairs(self.host.kp_off, d_prev, d_new, d_np)
        out.keep = (d_kl, d_cl)   # the launch may still be reading them
        return out


def matchToMap_batch_dev(ctx, inp, fmaxprojerr=2.0, fdistratio=0.2, fill=-7):
    """the device-resident form on arrays uploaded here.  Returns (match_cand, match_dist) after a synchronisation of its own."""
    d = MatchBatchInputDev(ctx, inp, fill)
    d.enqueue(fmaxprojerr, fdistratio)
    return d.get()


def random_brief_pattern(seed=0):
    """a 256 x 4 test table with the statistics of BRIEF's (isotropic Gaussian offsets, clipped to the patch): the real
    table of opencv_contrib is not in the reference tree"""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0, 48 / 5.0, (256, 4))), -24, 24).astype(np.int8)
