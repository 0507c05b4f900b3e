#!/usr/bin/env python3
"""times ov2_p3p_ransac_batch (P3P LMedS: solve / select / score / final launches) on synthetic 2D-3D scenes (GPU box),
and beside it, on batches of the same shape in the same session, the two stages it sits between: ov2_epipolar_filter_batch
(0 % outliers) and ov2_pnp_solve_batch.  Kernel times from ctx.kernel_timing, wall time of the host-pointer call."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, synth_ba, synth_epi, synth_p3p
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

ctx = fe.Context(0)
mvg = MultiViewGeometry(ctx)
P3P_KERNELS = ("p3p_solve_kernel", "p3p_select_kernel", "p3p_score_kernel", "p3p_final_kernel")


def timed(call):
    call()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ctx.kernel_timing(True)
    ctx.kernel_times()
    call()
    kt = ctx.kernel_times()
    ctx.kernel_timing(False)
    return min(ts) * 1e3, kt


def run_p3p(label, B, n, frac, lmeds=True, nmaxiter=100):
    scenes = [synth_p3p.make_scene(n, seed=100 * b + n, outlier_frac=frac, noise_px=0.3) for b in range(B)]
    args = ([s["bv"] for s in scenes], [s["wpts"] for s in scenes], nmaxiter, 3.0, np.array([s["K"] for s in scenes]),
            [17 * b + 1 for b in range(B)], lmeds)
    r = mvg.p3pRansac_batch(*args)
    wall, kt = timed(lambda: mvg.p3pRansac_batch(*args))
    k = [kt.get(name, (0, 0))[0] for name in P3P_KERNELS]
    tot = sum(k)
    print(f"p3p {label}: B={B} n={n} outliers={frac:.2f} kernels {tot:.3f} ms = solve {k[0]:.3f} + select {k[1]:.3f} + score {k[2]:.3f} "
          f"+ final {k[3]:.3f} ({B / (tot * 1e-3) if tot else 0:.0f} frames/s), wall {wall:.3f} ms, draws counted/skipped mean "
          f"{r['info'][:, 0].mean():.1f}/{r['info'][:, 1].mean():.1f}, status {np.bincount(r['status'], minlength=2).tolist()}", flush=True)


def run_neighbours(B, n):
    scenes = [synth_epi.make_scene(n, seed=100 * b + n, outlier_frac=0.0, baseline=0.5) for b in range(B)]
    args = ([s["bv_kf"] for s in scenes], [s["bv_cur"] for s in scenes], 100, 3.0, np.array([s["K"] for s in scenes]),
            [17 * b + 1 for b in range(B)])
    wall, kt = timed(lambda: mvg.compute5ptEssentialMatrix_batch(*args))
    print(f"epipolar: B={B} n={n} outliers=0.00 kernel {kt.get('epipolar_kernel', (0, 0))[0]:.3f} ms, wall {wall:.3f} ms", flush=True)
    q = [synth_ba.make_pnp(n, seed=b + 1) for b in range(B)]
    pargs = ([p["unpx"] for p in q], [p["wpts"] for p in q], np.array([p["Twc0"] for p in q]), 5, 5.9915, True, True,
             np.array([p["K"] for p in q]))
    wall, kt = timed(lambda: mvg.ceresPnP_batch(*pargs))
    print(f"pnp: B={B} n={n} kernel {kt.get('pnp_kernel', (0, 0))[0]:.3f} ms, wall {wall:.3f} ms", flush=True)


for B, n in ((64, 2048), (1, 308)):
    for frac in (0.0, 0.4):
        run_p3p("lmeds", B, n, frac)
    run_p3p("ransac", B, n, 0.4, lmeds=False)
    run_neighbours(B, n)
run_p3p("lmeds", 64, 308, 0.2)
run_p3p("lmeds", 256, 2048, 0.2)
run_p3p("lmeds", 1, 4096, 0.2)
run_p3p("lmeds", 1, 20000, 0.2)      # beyond the 4096 distances kept in LDS: recomputed per radix pass
