#!/usr/bin/env python3
"""device time of the keyframe detector chain (ov2_detect_grid_batch_dev, everything resident, nothing synchronised
inside) at bench.py's keyframe shape: B images, cell 13, 2048 grid keypoints thinned to 85 %, min-eig + cornerSubPix.
Prints the chain's time per call on an otherwise idle stream (hipEvents around N back-to-back calls: kernels + the gaps
between the chain's stream operations) and the per-kernel hipEvent averages of a separate instrumented pass."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
cell = 13
ctx = fe.Context(0)
S = synth.StereoStream()
ims = fe.Images(ctx, B, 752, 480)
for b in range(B):
    ims.upload(b, S.left(3 * (b % 8)))
pyr = fe.preprocess_images(ctx, ims)
base = synth.grid_keypoints(2048)
rng = np.random.default_rng(1)
cur = [base[rng.uniform(size=len(base)) < 0.85] for _ in range(B)]
cap = 2 * (752 // cell) * (480 // cell)
d_xy = ctx.to_device(np.concatenate(cur).astype(np.float32))
d_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(cur)]))
d_n, d_out = ctx.empty((B,), np.int32), ctx.empty((B, cap, 2), np.float32)
th0 = np.full(B, 0.001)
d_th0, d_th = ctx.to_device(th0), ctx.to_device(th0)
n_cur = sum(len(c) for c in cur)


def call():
    d_th.copy_from(d_th0)      # same thresholds every call: every call does the same work
    fe.detect_grid_batch_dev(ctx, pyr, cell, 1, d_th, n_cur, d_xy, d_img, None, d_n, d_out, cap)


for _ in range(20):
    call()
ctx.synchronize()
res = []
for _ in range(3):
    ctx.timer_start()
    for _ in range(N):
        call()
    res.append(1e3 * ctx.timer_stop() / N)
ctx.kernel_timing(True)
ctx.kernel_times()
for _ in range(50):
    call()
kt = ctx.kernel_times()
ctx.kernel_timing(False)
print(f"B={B} points={int(d_n.get().sum())}: chain "
      f"{min(res):.1f} us per call (runs {[round(r, 1) for r in res]}, incl. a {8 * B} B threshold copy); kernel averages us:",
      {k: round(1e3 * v[0] / max(v[1], 1), 2) for k, v in kt.items()}, flush=True)
