#!/usr/bin/env python3
"""times ov2_lcd_search2_batch_dev (the loop detector's exact word search alone, tables and arrays resident in HBM) on an
MI355X: one index of 50 k, 200 k and 1 M words against 600 queries, and 64 indices of 200 k words, 600 queries each; on the
same run ov2_knn2_hamming_batch_dev at 600 x 65 536, the only existing kernel to hold it against.
Device events around N back-to-back calls (each call = the search launch + the merge launch + the upload of the pair
descriptors); the shapes alternate inside each of ROUNDS rounds, so that the spread of a shape over the rounds is the
run-to-run noise its median is held against.  Prints the time per (query, word) compare of every shape and the VALU floor:
compares x VALU instructions per compare of the compiled inner loop / (CUs x 4 SIMDs x 16 lanes per clock x clock).
--out FILE also writes the figures as JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, lcd

ROUNDS = 7
VALU_PER_COMPARE = 24        # as knn2_kernel: 8 v_xor + 8 v_bcnt + 3 v_add3 + 5 (key, min / max, address moves)
CUS, CLOCK_GHZ = 256, 2.4    # MI355X
NQ = 600
# name, B, words per table, calls per window
SHAPES = (("lcd 1 x 50k", 1, 50_000, 400), ("lcd 1 x 200k", 1, 200_000, 200), ("lcd 1 x 1M", 1, 1_000_000, 60),
          ("lcd 64 x 200k", 64, 200_000, 4))
KNN = ("knn 600 x 65536", 1, 65536, 400)

ap = argparse.ArgumentParser()
ap.add_argument("--out")
args = ap.parse_args()
ctx = fe.Context(0)
rng = np.random.default_rng(0)
vp = lcd.vp


def rows(n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def window(call, n):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(n):
        assert call() == 0
    return ctx.timer_stop() / n * 1e3   # us per call


calls, keep = {}, []
big = lcd.Table(ctx, 1_000_000)
big.append(rows(1_000_000))
for name, B, words, n in SHAPES:
    if B == 1:
        t = big if words == 1_000_000 else lcd.Table(ctx, words)
        if t is not big:
            t.append(rows(words))
        tabs = [t]
    else:
        tabs = []
        for _ in range(B):
            t = lcd.Table(ctx, words)
            t.append(rows(words))
            tabs.append(t)
    keep.append(tabs)
    hs, nq = lcd._handles(tabs), np.full(B, NQ, np.int32)
    d_q, d_i, d_d = ctx.to_device(rows(B * NQ)), ctx.empty((B * NQ, 2), np.int32), ctx.empty((B * NQ, 2), np.int32)
    keep.append((hs, nq, d_q, d_i, d_d))
    calls[name] = (lambda B=B, hs=hs, nq=nq, d_q=d_q, d_i=d_i, d_d=d_d:
                   ctx.lib.ov2_lcd_search2_batch_dev(ctx.h, B, hs, nq.ctypes.data_as(vp), d_q.ptr, d_i.ptr, d_d.ptr), B * NQ * words, n)
name, B, words, n = KNN
qo, to = np.array([0, NQ], np.int32), np.array([0, words], np.int32)
dev = [ctx.to_device(a) for a in (qo, to, rows(NQ), rows(words), np.zeros((NQ, 2), np.int32), np.zeros((NQ, 2), np.int32))]
calls[name] = (lambda: ctx.lib.ov2_knn2_hamming_batch_dev(ctx.h, 1, NQ, *[d.ptr for d in dev]), NQ * words, n)

for name, (call, compares, n) in calls.items():   # warm up every shape
    window(call, 3)
t = {name: [] for name in calls}
for _ in range(ROUNDS):
    for name, (call, compares, n) in calls.items():
        t[name].append(window(call, n))
out = {}
for name, (call, compares, n) in calls.items():
    v = np.array(t[name])
    med = float(np.median(v))
    floor = compares * VALU_PER_COMPARE / (CUS * 4 * 16 * CLOCK_GHZ * 1e3)   # us
    out[name] = dict(median_us=med, min_us=float(v.min()), max_us=float(v.max()), compares=compares, ps_per_compare=med * 1e6 / compares,
                     valu_floor_us=floor)
    print(f"{name:16s}: median {med:10.2f} us  min {v.min():10.2f}  max {v.max():10.2f}  {med * 1e6 / compares:7.3f} ps per compare  "
          f"VALU floor {floor:9.2f} us  floor / median {floor / med:.3f}", flush=True)
r = out["lcd 1 x 50k"]["ps_per_compare"] / out[KNN[0]]["ps_per_compare"]
print(f"per-compare time, lcd at 50 k words / matcher at 65 536: {r:.2f}", flush=True)
# split counts at the largest single index: forced values around the automatic choice
call, compares, n = calls["lcd 1 x 1M"]
for splits in (0, 8, 26, 52, 103, 205, 410):
    lcd.set_splits(ctx, splits)
    window(call, 3)
    v = [window(call, 30) for _ in range(3)]
    out[f"lcd 1 x 1M splits {splits}"] = dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)))
    print(f"lcd 1 x 1M, splits {splits:4d}: median {np.median(v):10.2f} us  min {min(v):10.2f}  max {max(v):10.2f}", flush=True)
lcd.set_splits(ctx, 0)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
