#!/usr/bin/env python3
"""times ov2_match_to_map_batch (Mapper::matchToMap for B frames) on an MI355X at EuRoC size -- about 300 keypoints, a local
map of 2500 candidates and a keyframe table of 50 per frame -- against the per-keyframe entry point ov2_match_to_map on the
same frames in the same job:
  host form (staging, upload, launches, download, one synchronisation per call; host clock around the synchronise): 64
    ov2_match_to_map calls against one ov2_match_to_map_batch call of the same 64 frames, and one call of each on one frame;
    the variants alternate inside each of ROUNDS rounds after a warm-up (the spread over the rounds is the noise a median is
    held against);
  device form (arrays resident in HBM): device events around N back-to-back ov2_match_to_map_batch_dev calls, B = 1 and B = 64;
  per-kernel device time from ov2_ktime_report.
The outputs of the paths are compared at the sizes timed before anything is timed.  The 64 frames are 8 generated frames
repeated: a frame's result does not depend on its neighbours, and every copy has its own arrays."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, mapper, synth_match as SM

ROUNDS, B = 7, 64
GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)

ctx = fe.Context(0)
base = [SM.timing_frame(50 + i) for i in range(8)]
frames = [base[i % 8] for i in range(B)]
singles = [SM.single_input(f) for f in base]
batch = SM.batch_input(frames)
one = SM.batch_input(frames[:1])
d_batch, d_one = mapper.MatchBatchInputDev(ctx, batch), mapper.MatchBatchInputDev(ctx, one)

# same bits from every path before anything is timed
mc, md = mapper.matchToMap_batch(ctx, batch, *GATES)
d_batch.enqueue(*GATES)
dc, dd = d_batch.get()
assert mc.tobytes() == dc.tobytes() and md.tobytes() == dd.tobytes()
for b, (bc, bd) in enumerate(batch.split(mc, md)):
    sc, sd = mapper.matchToMap(ctx, singles[b % 8], *GATES)
    assert np.array_equal(sc, bc) and np.array_equal(sd, bd), b
d_one.enqueue(*GATES)
oc, od = d_one.get()
assert np.array_equal(oc, mc[:batch.kp_off[1]]) and np.array_equal(od, md[:batch.kp_off[1]])
print(f"{B} frames of {len(base[0]['kps'])} keypoints x {len(base[0]['cands'])} candidates x {len(base[0]['kf_Twc'])} keyframes: "
      f"{int((mc >= 0).sum())} matches, batch host form = batch device form = {B} ov2_match_to_map calls (bytewise)", flush=True)


def dev_window(fn, n):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(n):
        fn()
    return ctx.timer_stop() / n * 1e3   # us per repetition


def host_window(fn, n):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


K_SINGLES, K_BATCH = "host 64 ov2_match_to_map calls", "host one batch call, B=64"
host_variants = {K_SINGLES: (lambda: [mapper.matchToMap(ctx, singles[i % 8], *GATES) for i in range(B)], 3),
                 K_BATCH: (lambda: mapper.matchToMap_batch(ctx, batch, *GATES), 10),
                 "host one ov2_match_to_map call": (lambda: mapper.matchToMap(ctx, singles[0], *GATES), 100),
                 "host one batch call, B=1": (lambda: mapper.matchToMap_batch(ctx, one, *GATES), 100)}
dev_variants = {"dev  batch B=64, one call": (lambda: d_batch.enqueue(*GATES), 100),
                "dev  batch B=1, one call": (lambda: d_one.enqueue(*GATES), 500)}
t = {k: [] for k in list(host_variants) + list(dev_variants)}
for k, (fn, n) in host_variants.items():
    host_window(fn, 2)
for k, (fn, n) in dev_variants.items():
    dev_window(fn, 3)
for _ in range(ROUNDS):
    for k, (fn, n) in host_variants.items():
        t[k].append(host_window(fn, n))
    for k, (fn, n) in dev_variants.items():
        t[k].append(dev_window(fn, n))
for k, v in t.items():
    v = np.array(v)
    print(f"  {k:36s}: median {np.median(v):10.1f} us  min {v.min():10.1f}  max {v.max():10.1f}", flush=True)
ms, mb = np.median(t[K_SINGLES]), np.median(t[K_BATCH])
print(f"  64 single calls / one batch call (host wall time, medians): {ms / mb:.2f}x; per frame {ms / B:.1f} us -> {mb / B:.1f} us; "
      f"device time per frame, B=64: {np.median(t['dev  batch B=64, one call']) / B:.2f} us, B=1: "
      f"{np.median(t['dev  batch B=1, one call']):.2f} us", flush=True)

ctx.kernel_timing(True)
ctx.kernel_times()
for _ in range(50):
    d_batch.enqueue(*GATES)
kt = ctx.kernel_times()
print(f"  ktime match_kernels, batch B=64: {kt['match_kernels'][0] / 50 * 1e3:.1f} us per call ({kt['match_kernels'][1] // 50} launches)", flush=True)
for _ in range(50):
    mapper.matchToMap(ctx, singles[0], *GATES)
kt = ctx.kernel_times()
print(f"  ktime match_kernels, ov2_match_to_map on one frame: {kt['match_kernels'][0] / 50 * 1e3:.1f} us per call", flush=True)
ctx.kernel_timing(False)
assert max(t[K_BATCH]) < min(t[K_SINGLES]), "the batch call of 64 frames must take less wall time than the 64 single calls"
