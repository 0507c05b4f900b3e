"""ctypes binding of the loop closer's map matcher (ov2_loop_match_to_map_batch, include/ov2slam_hip.h):
  LoopCloser::matchToMap  src/loop_closer.cpp:586-763, B candidate pairs per call (flat inputs: LoopMatchInput)
Plumbing only (ctypes + numpy): the projections, gates and Hamming distances run in csrc/match.hip."""
import ctypes as C

import numpy as np

from .ba_types import CamModelC
from .mapper import _MatcherInput, _MatcherInputDev, _arrays, _csr, _host_call, f32p, f64p, i32p, u8p


class LoopMatchInputC(C.Structure):
    _fields_ = [("B", C.c_int32), ("n_kp", C.c_int32), ("n_cand", C.c_int32), ("K", C.c_double * 4), ("img_w", C.c_int32),
                ("img_h", C.c_int32), ("cell", C.c_int32), ("cam", C.c_void_p), ("Twc", f64p), ("kp_off", i32p), ("cand_off", i32p),
                ("kp_px", f32p), ("kp_matched", u8p), ("kp_desc_ptr", i32p), ("kp_descs", u8p), ("kp_kf_ptr", i32p),
                ("kp_kfids", i32p), ("grid_ptr", i32p), ("grid_kp", i32p), ("cand_wpt", f64p), ("cand_desc_ptr", i32p),
                ("cand_descs", u8p), ("cand_kf_ptr", i32p), ("cand_kfids", i32p)]


ARRAYS = _arrays(LoopMatchInputC)


class LoopMatchInput(_MatcherInput):
    """owns the flat arrays of one ov2_loop_match_to_map_batch call.
    pairs: list of dict(Twc (7,), kps, cands); kps: list of dict(px (2,), matched bool, descs (d,32) u8 -- empty where the
    keypoint's map point is gone or has no descriptor --, kfids [ascending]); cands: list of dict(wpt (3,), descs, kfids), in the
    order the caller walks the local map.  Each pair's grid (Frame::vgridkps_) is rebuilt from its kp order = insertion order.
    cam: None or ba_types.CamModelC (one camera per call)."""

    def __init__(self, pairs, K, img_w, img_h, cell, cam=None):
        kps = self._build(pairs, img_w, img_h, cell)
        self.Twc = np.ascontiguousarray([p["Twc"] for p in pairs], np.float64).reshape(-1, 7)
        self.kp_matched = np.ascontiguousarray([bool(k["matched"]) for k in kps], np.uint8)
        m = LoopMatchInputC()
        m.B = len(pairs)
        self._fill(m, K, img_w, img_h, cell, cam)


def loopMatchToMap_batch(ctx, inp, fmaxprojerr=10.0, fdistratio=0.2):
    """host form.  returns (match_cand (n_kp,) int32: candidate index within the pair or -1, match_dist (n_kp,) f32); slice them
    with inp.kp_off"""
    return _host_call(ctx, "ov2_loop_match_to_map_batch", inp, fmaxprojerr, fdistratio)


class LoopMatchInputDev(_MatcherInputDev):
    """a LoopMatchInput resident in HBM, for ov2_loop_match_to_map_batch_dev"""
    ENTRY, FMAXPROJERR = "ov2_loop_match_to_map_batch_dev", 10.0


def loopMatchToMap_batch_dev(ctx, inp, fmaxprojerr=10.0, fdistratio=0.2, fill=-7):
    """the device-resident form on arrays uploaded here.  Returns (match_cand, match_dist) after a synchronisation of its own."""
    d = LoopMatchInputDev(ctx, inp, fill)
    d.enqueue(fmaxprojerr, fdistratio)
    return d.get()
