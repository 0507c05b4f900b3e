#!/usr/bin/env python3
"""times ov2_epipolar_filter_batch (5-point RANSAC + Sampson gate, one workgroup per frame) on synthetic two-view scenes
(GPU box): kernel time from ctx.kernel_timing, wall time of the host-pointer call, OpenGV iterations per frame."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, synth_epi
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

ctx = fe.Context(0)
mvg = MultiViewGeometry(ctx)


def run(label, B, scenes, nmaxiter=100):
    args = ([s["bv_kf"] for s in scenes], [s["bv_cur"] for s in scenes], nmaxiter, 3.0, np.array([s["K"] for s in scenes]),
            [17 * b + 1 for b in range(B)], [s["gate_kf"] for s in scenes], [s["gate_cur"] for s in scenes])
    r = mvg.compute5ptEssentialMatrix_batch(*args)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        mvg.compute5ptEssentialMatrix_batch(*args)
        ts.append(time.perf_counter() - t0)
    ctx.kernel_timing(True)
    ctx.kernel_times()
    mvg.compute5ptEssentialMatrix_batch(*args)
    kt = ctx.kernel_times()
    ctx.kernel_timing(False)
    k = kt.get("epipolar_kernel", (0, 0))[0]
    it = r["info"][:, 0] + r["info"][:, 1]
    print(f"{label}: B={B} kernel {k:.3f} ms ({B / (k * 1e-3) if k else 0:.0f} frames/s), wall {min(ts) * 1e3:.3f} ms, "
          f"draws/frame max {it.max()} mean {it.mean():.1f}, status {np.bincount(r['status'], minlength=3).tolist()}",
          flush=True)


for B in (1, 8, 64):
    for n in (308, 2048):
        for frac in (0.0, 0.2, 0.45):
            scenes = [synth_epi.make_scene(n, seed=100 * b + n, outlier_frac=frac, baseline=0.5, n_gate=n // 4)
                      for b in range(B)]
            run(f"n={n} outliers={frac:.2f}", B, scenes)
# worst cases: pure noise (the iteration cap), a degenerate frame (every draw skipped: 10 nmaxiter draws)
rng = np.random.default_rng(5)
for B in (1, 64):
    scenes = []
    for b in range(B):
        s = synth_epi.make_scene(2048, seed=b, outlier_frac=0.0, baseline=0.5)
        v = rng.normal(size=(2048, 3)) + [0, 0, 3]
        s["bv_cur"] = v / np.linalg.norm(v, axis=1, keepdims=True)
        scenes.append(s)
    run("n=2048 pure noise", B, scenes)
    scenes = []
    for b in range(B):
        s = synth_epi.make_scene(2048, seed=b, outlier_frac=0.0, baseline=0.5)
        s["bv_kf"][:] = s["bv_kf"][0]
        s["bv_cur"][:] = s["bv_cur"][0]
        scenes.append(s)
    run("n=2048 degenerate (all pairs equal)", B, scenes)
