#!/usr/bin/env python3
"""times ov2_fast_detect_batch_dev (whole-image FAST + NMS + mask + retainBest, everything resident in HBM) and the same
followed by ov2_describe_brief_dev on its keypoints, on an MI355X: B = 1 and B = 64 raw images of 752 x 480 (seeded blocks with
noise, about 300 mask points each, threshold 20, mask radius 2, n_best 300).
Device events around N back-to-back calls; the shapes alternate inside each of ROUNDS rounds, so that the spread of a shape over
the rounds is the run-to-run noise its median is held against.  Then the per-kernel split from ov2_ktime_report, and the memory
floor: image bytes read once plus score bytes written and read, over the HBM bandwidth.  --out FILE also writes JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, mapper, synth_fast as S

ROUNDS = 7
W, H, N_MASK, CAP = 752, 480, 300, 2048
HBM_GBS = 8000.0   # MI355X peak
SHAPES = (("B = 1", 1, 200), ("B = 64", 64, 10))

ap = argparse.ArgumentParser()
ap.add_argument("--out")
args = ap.parse_args()
ctx = fe.Context(0)


def window(call, n):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(n):
        call()
    return ctx.timer_stop() / n * 1e3   # us per call


calls, keep = {}, []
d_pat = ctx.to_device(mapper.random_brief_pattern(3))
for name, B, n in SHAPES:
    im = fe.Images(ctx, B, W, H)
    for b in range(B):
        im.upload(b, S.noise_blocks_image(W, H, seed=b))
    pyr = fe.preprocess_images(ctx, im, use_clahe=False, nklt_pyr_lvl=0)
    xy = np.concatenate([S.mask_points(W, H, N_MASK, seed=100 + b) for b in range(B)])
    idx = np.repeat(np.arange(B, dtype=np.int32), N_MASK)
    d = dict(xy=ctx.to_device(xy), idx=ctx.to_device(idx), nt=ctx.empty(B, np.int32), no=ctx.empty(B, np.int32),
             oxy=ctx.empty((B, CAP, 2), np.float32), orr=ctx.empty((B, CAP), np.uint8))
    detect = (lambda pyr=pyr, d=d, B=B: fe.fast_detect_batch_dev(ctx, pyr, 20, 2, B * N_MASK, d["xy"], d["idx"], 300, CAP, d["nt"], d["no"],
                                                                 d["oxy"], d["orr"]))
    detect()
    ctx.synchronize()
    n_out = d["no"].get()
    # the describe call of the timing: the first 300 places of every image (the counts stay on the device in the _dev chain)
    take = 300
    assert n_out.min() >= take, n_out.min()
    pts = ctx.to_device(d["oxy"].get()[:, :take].reshape(-1, 2))
    pidx = ctx.to_device(np.repeat(np.arange(B, dtype=np.int32), take))
    desc, valid = ctx.empty((B * take, 32), np.uint8), ctx.empty(B * take, np.uint8)

    def both(detect=detect, pyr=pyr, pts=pts, pidx=pidx, desc=desc, valid=valid, B=B):
        detect()
        assert ctx.lib.ov2_describe_brief_dev(ctx.h, pyr.h, B * take, pts.ptr, pidx.ptr, d_pat.ptr, desc.ptr, valid.ptr) == 0

    keep.append((im, pyr, d, pts, pidx, desc, valid))
    calls[f"detect, {name}"] = (detect, B, n)
    calls[f"detect + describe, {name}"] = (both, B, n)
    print(f"{name}: keypoints kept per image {d['nt'].get().min()} .. {d['nt'].get().max()}", flush=True)

for name, (call, B, n) in calls.items():   # warm up every shape
    window(call, 3)
t = {name: [] for name in calls}
for _ in range(ROUNDS):
    for name, (call, B, n) in calls.items():
        t[name].append(window(call, n))
out = {}
for name, (call, B, n) in calls.items():
    v = np.array(t[name])
    med = float(np.median(v))
    floor = B * 3.0 * W * H / (HBM_GBS * 1e3)   # us: image read once, score plane written and read
    out[name] = dict(median_us=med, min_us=float(v.min()), max_us=float(v.max()), us_per_image=med / B, hbm_floor_us=floor)
    print(f"{name:28s}: median {med:9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  {med / B:8.2f} us per image  "
          f"HBM floor {floor:8.2f} us  floor / median {floor / med:.3f}", flush=True)
# per-kernel split of one shape at a time
ctx.kernel_timing(True)
for name, (call, B, n) in calls.items():
    if not name.startswith("detect + describe"):
        continue
    ctx.kernel_times()
    for _ in range(n):
        call()
    kt = ctx.kernel_times()
    out[name]["kernels_us_per_call"] = {k: v[0] / n * 1e3 for k, v in kt.items()}
    print(f"{name}: " + ", ".join(f"{k} {v[0] / n * 1e3:.2f} us ({v[1] // n} launches)" for k, v in kt.items()), flush=True)
ctx.kernel_timing(False)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
