"""ctypes binding of the loop closer's map matcher (ov2_loop_match_to_map_batch, include/ov2slam_hip.h):
  LoopCloser::matchToMap  src/loop_closer.cpp:586-763, B candidate pairs per call (flat inputs: LoopMatchInput)
Plumbing only (ctypes + numpy): the projections, gates and Hamming distances run in csrc/match.hip."""
import ctypes as C

import numpy as np

from .ba_types import CamModelC
from .frontend import _check
from .mapper import _csr, f32p, f64p, i32p, u8p


class LoopMatchInputC(C.Structure):
    _fields_ = [("B", C.c_int32), ("n_kp", C.c_int32), ("n_cand", C.c_int32), ("K", C.c_double * 4), ("img_w", C.c_int32),
                ("img_h", C.c_int32), ("cell", C.c_int32), ("cam", C.c_void_p), ("Twc", f64p), ("kp_off", i32p), ("cand_off", i32p),
                ("kp_px", f32p), ("kp_matched", u8p), ("kp_desc_ptr", i32p), ("kp_descs", u8p), ("kp_kf_ptr", i32p),
                ("kp_kfids", i32p), ("grid_ptr", i32p), ("grid_kp", i32p), ("cand_wpt", f64p), ("cand_desc_ptr", i32p),
                ("cand_descs", u8p), ("cand_kf_ptr", i32p), ("cand_kfids", i32p)]


ARRAYS = (("Twc", f64p), ("kp_off", i32p), ("cand_off", i32p), ("kp_px", f32p), ("kp_matched", u8p), ("kp_desc_ptr", i32p),
          ("kp_descs", u8p), ("kp_kf_ptr", i32p), ("kp_kfids", i32p), ("grid_ptr", i32p), ("grid_kp", i32p), ("cand_wpt", f64p),
          ("cand_desc_ptr", i32p), ("cand_descs", u8p), ("cand_kf_ptr", i32p), ("cand_kfids", i32p))


class LoopMatchInput:
    """owns the flat arrays of one ov2_loop_match_to_map_batch call.
    pairs: list of dict(Twc (7,), kps, cands); kps: list of dict(px (2,), matched bool, descs (d,32) u8 -- empty where the
    keypoint's map point is gone or has no descriptor --, kfids [ascending]); cands: list of dict(wpt (3,), descs, kfids), in the
    order the caller walks the local map.  Each pair's grid (Frame::vgridkps_) is rebuilt from its kp order = insertion order.
    cam: None or ba_types.CamModelC (one camera per call)."""

    def __init__(self, pairs, K, img_w, img_h, cell, cam=None):
        c = np.ascontiguousarray
        B = len(pairs)
        kps = [k for p in pairs for k in p["kps"]]
        cands = [q for p in pairs for q in p["cands"]]
        self.Twc = c([p["Twc"] for p in pairs], np.float64).reshape(-1, 7)
        self.kp_off = np.concatenate([[0], np.cumsum([len(p["kps"]) for p in pairs])]).astype(np.int32)
        self.cand_off = np.concatenate([[0], np.cumsum([len(p["cands"]) for p in pairs])]).astype(np.int32)
        self.kp_px = c([k["px"] for k in kps], np.float32).reshape(-1, 2)
        self.kp_matched = c([bool(k["matched"]) for k in kps], np.uint8)
        self.kp_desc_ptr, self.kp_descs = _csr([k["descs"] for k in kps], np.uint8, 32)
        self.kp_kf_ptr, self.kp_kfids = _csr([k["kfids"] for k in kps], np.int32)
        nbw, nbh = int(np.ceil(np.float32(img_w) / np.float32(cell))), int(np.ceil(np.float32(img_h) / np.float32(cell)))
        cells = [[] for _ in range(B * nbw * nbh)]
        for b, p in enumerate(pairs):
            for i, k in enumerate(p["kps"]):
                r = int(np.floor(np.float32(k["px"][1]) / np.float32(cell)))
                cc = int(np.floor(np.float32(k["px"][0]) / np.float32(cell)))
                cells[b * nbw * nbh + r * nbw + cc].append(i)
        self.grid_ptr, self.grid_kp = _csr(cells, np.int32)
        self.cand_wpt = c([q["wpt"] for q in cands], np.float64).reshape(-1, 3)
        self.cand_desc_ptr, self.cand_descs = _csr([q["descs"] for q in cands], np.uint8, 32)
        self.cand_kf_ptr, self.cand_kfids = _csr([q["kfids"] for q in cands], np.int32)
        self.cam = cam
        m = LoopMatchInputC()
        m.B, m.n_kp, m.n_cand = B, len(kps), len(cands)
        m.K[:] = np.asarray(K, np.float64).tolist()
        m.img_w, m.img_h, m.cell = int(img_w), int(img_h), int(cell)
        m.cam = None if cam is None else C.addressof(cam)
        for name, t in ARRAYS:
            setattr(m, name, getattr(self, name).ctypes.data_as(t))
        self.c = m


def loopMatchToMap_batch(ctx, inp, fmaxprojerr=10.0, fdistratio=0.2):
    """host form.  returns (match_cand (n_kp,) int32: candidate index within the pair or -1, match_dist (n_kp,) f32); slice them
    with inp.kp_off"""
    n = inp.c.n_kp
    mc, md = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.float32)
    _check(ctx.h, ctx.lib.ov2_loop_match_to_map_batch(ctx.h, C.addressof(inp.c), float(fmaxprojerr), float(fdistratio), mc.ctypes.data,
                                                      md.ctypes.data))
    return mc[:n], md[:n]


class LoopMatchInputDev:
    """a LoopMatchInput resident in HBM, with the work and output arrays of ov2_loop_match_to_map_batch_dev; the outputs start
    as `fill` so that untouched slots show"""

    def __init__(self, ctx, inp, fill=-7):
        self.ctx, self.host, n = ctx, inp, inp.c.n_kp
        self.dev = {name: ctx.to_device(getattr(inp, name)) for name, _ in ARRAYS}
        self.c = LoopMatchInputC()
        C.memmove(C.addressof(self.c), C.addressof(inp.c), C.sizeof(self.c))
        for name, t in ARRAYS:
            setattr(self.c, name, C.cast(self.dev[name].ptr, t))
        self.d_work = ctx.to_device(np.zeros(max(n, 1), np.uint64))
        self.d_mc, self.d_md = ctx.to_device(np.full(max(n, 1), fill, np.int32)), ctx.to_device(np.full(max(n, 1), fill, np.float32))

    def enqueue(self, fmaxprojerr=10.0, fdistratio=0.2):
        """asynchronous: nothing is synchronised"""
        _check(self.ctx.h, self.ctx.lib.ov2_loop_match_to_map_batch_dev(self.ctx.h, C.addressof(self.c), float(fmaxprojerr),
                                                                        float(fdistratio), self.d_work.ptr, self.d_mc.ptr, self.d_md.ptr))

    def get(self):
        n = self.host.c.n_kp
        self.ctx.synchronize()
        return self.d_mc.get()[:n], self.d_md.get()[:n]


def loopMatchToMap_batch_dev(ctx, inp, fmaxprojerr=10.0, fdistratio=0.2, fill=-7):
    """the device-resident form on arrays uploaded here.  Returns (match_cand, match_dist) after a synchronisation of its own."""
    d = LoopMatchInputDev(ctx, inp, fill)
    d.enqueue(fmaxprojerr, fdistratio)
    return d.get()
