#!/usr/bin/env python3
"""times ov2_loop_match_to_map_batch (LoopCloser::matchToMap for B pairs) on an MI355X at EuRoC size -- about 300 keypoints
and 2000 local-map points per pair -- for 64 pairs and for one:
  device form (arrays resident in HBM): one call with B = 64, 64 calls with B = 1, one call with B = 1; device events around
    N back-to-back calls, the variants alternating inside each of ROUNDS rounds (the spread over the rounds is the noise a
    median is held against);
  host form (staging, upload, launch, download, one synchronisation): B = 64, B = 1, and one ov2_match_to_map call
    (Mapper::matchToMap, the single-frame matcher with its mean-reprojection gate) on the same keypoints and candidates;
    host clock, the call synchronises;
  per-kernel device time of both matchers from ov2_ktime_report.
The 64 pairs are 8 generated pairs repeated: a pair's result does not depend on its neighbours, and every copy has its own
arrays."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, loop_match as LM, mapper, synth_revisit as SR

ROUNDS, N_KP, N_CAND, B = 7, 300, 2000, 64
GATES = (SR.FMAXPROJERR, SR.FDISTRATIO)
CAMERA = (SR.K4, SR.W, SR.H, SR.CELL)

ctx = fe.Context(0)
rng = np.random.default_rng(0)
base = [SR._general(rng, 1000 * (i + 1), n_kp=N_KP, n_cand=N_CAND).dict() for i in range(8)]
pairs = [base[i % 8] for i in range(B)]
batch = LM.LoopMatchInput(pairs, *CAMERA)
singles = [LM.LoopMatchInput([p], *CAMERA) for p in base]
d_batch = LM.LoopMatchInputDev(ctx, batch)
d_singles = [LM.LoopMatchInputDev(ctx, s) for s in singles]

# same bits from every form before anything is timed
mc, md = LM.loopMatchToMap_batch(ctx, batch, *GATES)
d_batch.enqueue(*GATES)
dc, dd = d_batch.get()
assert mc.tobytes() == dc.tobytes() and md.tobytes() == dd.tobytes()
for i, d in enumerate(d_singles):
    d.enqueue(*GATES)
    sc, sd = d.get()
    assert np.array_equal(sc, mc[batch.kp_off[i]:batch.kp_off[i + 1]]) and np.array_equal(sd, md[batch.kp_off[i]:batch.kp_off[i + 1]])
print(f"{B} pairs of {N_KP} keypoints x {N_CAND} local-map points: {int((mc >= 0).sum())} matches, "
      f"host form = device form = single-pair calls (bytewise)", flush=True)


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


def all_singles():
    for i in range(B):
        d_singles[i % 8].enqueue(*GATES)


# Mapper::matchToMap on pair 0: its extra inputs (pixels in the keypoint's keyframes, keyframe poses) are set so that the
# mean-reprojection gate passes wherever the pixel gate does; nb3dkps >= 30 keeps dmaxpxdist undoubled
p0 = base[0]
kps0 = [dict(px=k["px"], descs=k["descs"], kfids=k["kfids"], kf_px=np.tile(k["px"], (len(k["kfids"]), 1))) for k in p0["kps"]]
old = mapper.MatchInput(p0["Twc"], SR.K4, SR.W, SR.H, SR.CELL, 120, kps0, p0["cands"], np.tile(p0["Twc"], (45, 1)))

dev_variants = {"dev  B=64, one call": (lambda: d_batch.enqueue(*GATES), 200),
                "dev  64 calls of B=1": (all_singles, 20),
                "dev  B=1, one call": (lambda: d_singles[0].enqueue(*GATES), 1000)}
host_variants = {"host B=64, one call": (lambda: LM.loopMatchToMap_batch(ctx, batch, *GATES), 20),
                 "host 64 calls of B=1": (lambda: [LM.loopMatchToMap_batch(ctx, singles[i % 8], *GATES) for i in range(B)], 3),
                 "host B=1, one call": (lambda: LM.loopMatchToMap_batch(ctx, singles[0], *GATES), 200),
                 "host ov2_match_to_map, same shape": (lambda: mapper.matchToMap(ctx, old, SR.FMAXPROJERR, SR.FDISTRATIO), 200)}
t = {k: [] for k in list(dev_variants) + list(host_variants)}
for k, (fn, n) in dev_variants.items():
    dev_window(fn, 3)
for k, (fn, n) in host_variants.items():
    host_window(fn, 2)
for _ in range(ROUNDS):
    for k, (fn, n) in dev_variants.items():
        t[k].append(dev_window(fn, n))
    for k, (fn, n) in host_variants.items():
        t[k].append(host_window(fn, n))
for k, v in t.items():
    v = np.array(v)
    print(f"  {k:36s}: median {np.median(v):10.1f} us  min {v.min():10.1f}  max {v.max():10.1f}", flush=True)

ctx.kernel_timing(True)
ctx.kernel_times()
for _ in range(50):
    d_batch.enqueue(*GATES)
kt = ctx.kernel_times()
print(f"  ktime loop_match_kernels, B=64: {kt['loop_match_kernels'][0] / 50 * 1e3:.1f} us per call ({kt['loop_match_kernels'][1] // 50} launches)", flush=True)
for _ in range(50):
    d_singles[0].enqueue(*GATES)
kt = ctx.kernel_times()
print(f"  ktime loop_match_kernels, B=1 : {kt['loop_match_kernels'][0] / 50 * 1e3:.1f} us per call", flush=True)
for _ in range(50):
    mapper.matchToMap(ctx, old, SR.FMAXPROJERR, SR.FDISTRATIO)
kt = ctx.kernel_times()
print(f"  ktime match_kernels (ov2_match_to_map), same shape: {kt['match_kernels'][0] / 50 * 1e3:.1f} us per call", flush=True)
ctx.kernel_timing(False)
