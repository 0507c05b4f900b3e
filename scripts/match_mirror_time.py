#!/usr/bin/env python3
"""times local-map matching FROM THE MAP MIRRORS (ov2_map_match_local_batch: device-side gather of the matcher's input, then the
matcher's own kernels) on an MI355X against the host-pointer form ov2_match_to_map_batch on the same frames in the same job.

Workload: 64 maps of synth_match.timing_frame size (300 keypoints x 2500 candidates, 50 keyframes), each a mirror of its own with
the match columns (8 generated frames repeated; every copy has its own tables).  A frame becomes a map like this: keyframes 0..49,
the new keyframe 49; keypoint i is landmark i, observed by the new keyframe at its pixel and by its listed keyframes at their
pixels; candidate c is landmark n_kp + c, observed by its listed keyframes; a descriptor sits on the row of the keyframe it is
listed with, while there are rows.  The host-pointer form runs on the arrays the gather itself produces (downloaded once), so both
forms see the same frames, and their matches are compared before anything is timed.

Reported (medians over ROUNDS rounds after a warm-up; inside a round the two host forms alternate, and the order flips every
round):
  wall time per call, host clock around a call that ends in its one synchronisation: mirror form, host-pointer form;
  bytes the caller hands over per call in either form;
  device time of the gather alone: device events around N back-to-back ov2_map_match_gather_batch_dev calls (upload included),
    and the summed kernel time of its launches from ov2_ktime_report."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, mapper, synth_match as SM

ROUNDS, B = 9, 64
GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)


def mirror_of(ctx, f):
    """a timing frame as a map mirror: (DeviceMap, keypoint lmids, candidate lmids)"""
    n_kf, n_kp, n_c = len(f["kf_Twc"]), len(f["kps"]), len(f["cands"])
    newkf = n_kf - 1
    rows = {k: [] for k in range(n_kf)}     # kfid -> (lmid, px, desc or None)
    for i, k in enumerate(f["kps"]):
        rows[newkf].append((i, k["px"], None))
        for j, kf in enumerate(k["kfids"]):
            rows[kf].append((i, k["kf_px"][j], k["descs"][j] if j < len(k["descs"]) else None))
    for c, q in enumerate(f["cands"]):
        for j, kf in enumerate(q["kfids"]):
            rows[kf].append((n_kp + c, np.zeros(2, np.float32), q["descs"][j] if j < len(q["descs"]) else None))
    m = DM.DeviceMap(ctx, n_kf + 2, n_kp + n_c + 2, sum(len(r) for r in rows.values()) + 16)
    m.enable_match_columns()
    m.newkf = newkf
    for kf, r in rows.items():
        lm = np.array([x[0] for x in r], np.int32)
        px = np.array([x[1] for x in r], np.float32).reshape(-1, 2)
        has = np.array([x[2] is not None for x in r], np.uint8)
        desc = np.array([x[2] if x[2] is not None else np.zeros(32, np.uint8) for x in r], np.uint8).reshape(-1, 32)
        m.add_keyframe_px(kf, f["kf_Twc"][kf], lm, px.astype(np.float64), px, desc, has)
    xyz = np.zeros((n_kp + n_c, 3))
    xyz[n_kp:] = [q["wpt"] for q in f["cands"]]
    m.set_landmarks(np.arange(n_kp + n_c, dtype=np.int32), xyz, np.full(n_kp + n_c, DM.LM_ALIVE | DM.LM_3D | DM.LM_KP3D, np.uint8))
    return m, list(range(n_kp)), list(range(n_kp, n_kp + n_c))


class FlatInput(mapper._MatcherInput):
    """the arrays a gather produced (device_map.match_gather_batch) as a host-pointer ov2_match_batch_input"""

    def __init__(self, g, K, img_w, img_h, cell):
        for name, t in mapper.BATCH_ARRAYS:
            setattr(self, name, np.ascontiguousarray(g[name]))
        m = mapper.MatchBatchInputC()
        m.B = g["B"]
        self._fill(m, K, img_w, img_h, cell, None)

    split = mapper.MatchBatchInput.split


def host_window(fn, n):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def dev_window(fn, n):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(n):
        fn()
    return ctx.timer_stop() / n * 1e3


ctx = fe.Context(0)
base = [SM.timing_frame(50 + i) for i in range(8)]
built = [mirror_of(ctx, base[b % 8]) for b in range(B)]
maps, kps, cands = [x[0] for x in built], [x[1] for x in built], [x[2] for x in built]
grid = SM.batch_input([base[b % 8] for b in range(B)])      # the frames' own grids: keypoint order = insertion order
ids = dict(newkf=[m.newkf for m in maps], nb3dkps=[SM.NB3D] * B, kp_lists=kps, grids=(grid.grid_ptr, grid.grid_kp), cand_lists=cands,
           camera=SM.CAMERA)

g = DM.match_gather_batch(ctx, maps, **ids)
flat = FlatInput(g, *SM.CAMERA)
mc, md = mapper.matchToMap_batch(ctx, flat, *GATES)
res = DM.match_local_batch(ctx, maps, **ids, fmaxprojerr=GATES[0], fdistratio=GATES[1])
for b, ((bc, bd), (ml, dl)) in enumerate(zip(flat.split(mc, md), res)):
    want = np.where(bc >= 0, np.asarray(cands[b])[np.maximum(bc, 0)], -1)
    assert np.array_equal(want, ml) and np.array_equal(bd, dl), b
up_host = sum(getattr(flat, name).nbytes for name, _ in mapper.BATCH_ARRAYS)
a = DM._match_ids(maps, **{k: ids[k] for k in ("newkf", "nb3dkps", "kp_lists", "grids", "cand_lists")})
up_mirror = sum(a[k].nbytes for k in ("newkf", "nb3dkps", "kp_off", "kp_lmid", "cand_off", "cand_lmid", "grid_ptr", "grid_kp"))
print(f"{B} maps of {len(kps[0])} keypoints x {len(cands[0])} candidates x {len(base[0]['kf_Twc'])} keyframes, {sum(m.rows()[0] for m in maps)} rows: "
      f"{int((mc >= 0).sum())} matches, mirror form = host-pointer form on the gathered arrays (lmids and distances)", flush=True)
print(f"  the caller hands over per call: host-pointer form {up_host / 1e6:.2f} MB, mirror form {up_mirror / 1e6:.2f} MB", flush=True)

# raw calls on arguments built once, so that neither side's Python assembly is in the window
args = DM._match_call_args(ctx, a, SM.CAMERA, None)
n = int(a["kp_off"][-1])
ml, mdl = np.zeros(n, np.int32), np.zeros(n, np.float32)
hc, hd = np.zeros(n, np.int32), np.zeros(n, np.float32)
out_in, dk, dc = mapper.MatchBatchInputC(), C.c_void_p(), C.c_void_p()


def call_mirror():
    assert ctx.lib.ov2_map_match_local_batch(*args, GATES[0], GATES[1], ml.ctypes.data_as(C.c_void_p), mdl.ctypes.data_as(C.c_void_p)) == 0


def call_host():
    assert ctx.lib.ov2_match_to_map_batch(ctx.h, C.addressof(flat.c), GATES[0], GATES[1], hc.ctypes.data, hd.ctypes.data) == 0


def call_gather():
    assert ctx.lib.ov2_map_match_gather_batch_dev(*args, C.byref(out_in), C.byref(dk), C.byref(dc)) == 0


K_M, K_H = "mirror form  ov2_map_match_local_batch, B=64", "host-pointer ov2_match_to_map_batch,   B=64"
variants = {K_M: (call_mirror, 20), K_H: (call_host, 20)}
t = {k: [] for k in variants}
t_gather = []
for fn, _ in variants.values():
    host_window(fn, 3)
dev_window(call_gather, 5)
for r in range(ROUNDS):
    order = list(variants) if r % 2 == 0 else list(variants)[::-1]
    for k in order:
        t[k].append(host_window(*variants[k]))
    t_gather.append(dev_window(call_gather, 50))
assert np.array_equal(ml, np.concatenate([x[0] for x in res])) and np.array_equal(hc, mc)
for k, v in list(t.items()) + [("gather alone, device events (upload + 12 launches)", t_gather)]:
    v = np.array(v)
    print(f"  {k:52s}: median {np.median(v):9.1f} us  min {v.min():9.1f}  max {v.max():9.1f}", flush=True)
tm, th = np.median(t[K_M]), np.median(t[K_H])
print(f"  mirror / host-pointer wall time (medians): {tm / th:.2f}x; per frame {th / B:.1f} us -> {tm / B:.1f} us", flush=True)

ctx.kernel_timing(True)
ctx.kernel_times()
for _ in range(50):
    call_gather()
kt = ctx.kernel_times()
print(f"  ktime map_setup_kernels, gather B=64: {kt['map_setup_kernels'][0] / 50 * 1e3:.1f} us per call "
      f"({kt['map_setup_kernels'][1] // 50} launches)", flush=True)
for _ in range(50):
    call_host()
kt = ctx.kernel_times()
print(f"  ktime match_kernels, B=64: {kt['match_kernels'][0] / 50 * 1e3:.1f} us per call", flush=True)
ctx.kernel_timing(False)
for m in maps:
    m.close()
