#!/usr/bin/env python3
"""times the four library stages of LoopCloser::verifyLoopCandidates on an MI355X at EuRoC size, for 64 pairs and for one:
  P3P RANSAC      ov2_p3p_ransac_batch, use_lmeds = 0, 10 * nransac_iter = 1000 draws, 300 correspondences per pair, 20 % outliers
  refinement      ov2_pnp_solve_batch on the RANSAC inliers (K = (fx, fy, 0, 0), 10 iterations, robust, no L2 re-solve)
  local-map match ov2_loop_match_to_map_batch, 300 keypoints x 2000 local-map points per pair
  computePnP      ov2_pnp_solve_batch on 300 pairs (10 iterations, robust, no L2 re-solve)
Every stage is called through the host-pointer ABI as the host mirror calls it: wall time of the call (it ends in its
synchronisation, best of 3 after a warm-up) and the device time of its kernels from ov2_ktime_report.  The stages get
synthetic inputs of the right shape each (the host mirror's own bookkeeping is not timed); scripts/loop_match_time.py holds the
matcher against single-pair calls and against ov2_match_to_map."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, loop_match as LM, synth_ba, synth_p3p, synth_revisit as SR
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

N_CORR, N_KP, N_CAND, NRANSAC_ITER = 300, 300, 2000, 100
ctx = fe.Context(0)
mvg = MultiViewGeometry(ctx)


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
    return min(ts) * 1e3, sum(v[0] for v in kt.values()), {k: round(v[0], 4) for k, v in kt.items() if v[1]}


rng = np.random.default_rng(0)
base = [SR._general(rng, 1000 * (i + 1), n_kp=N_KP, n_cand=N_CAND).dict() for i in range(8)]
for B in (64, 1):
    sc = [synth_p3p.make_scene(N_CORR, seed=100 * b + 7, outlier_frac=0.2, noise_px=0.3) for b in range(B)]
    K = np.array([[s["K"][0], s["K"][1], 0., 0.] for s in sc])
    p3p = lambda: mvg.p3pRansac_batch([s["bv"] for s in sc], [s["wpts"] for s in sc], 10 * NRANSAC_ITER, 3.0, K, [17 * b + 1 for b in range(B)], False)
    r = p3p()
    assert (r["status"] == 1).all()
    inl = [~o & (s["bv"][:, 2] > 0) for o, s in zip(r["outlier"], sc)]
    unpx = [np.stack([k[0] * s["bv"][m, 0] / s["bv"][m, 2], k[1] * s["bv"][m, 1] / s["bv"][m, 2]], 1) for s, m, k in zip(sc, inl, K)]
    refine = lambda: mvg.ceresPnP_batch(unpx, [s["wpts"][m] for s, m in zip(sc, inl)], r["Twc"], 10, 5.9915, True, False, K)
    assert refine()[0].all()
    match_in = LM.LoopMatchInput([base[i % 8] for i in range(B)], SR.K4, SR.W, SR.H, SR.CELL)
    match = lambda: LM.loopMatchToMap_batch(ctx, match_in, SR.FMAXPROJERR, SR.FDISTRATIO)
    pn = [synth_ba.make_pnp(N_CORR, seed=50 + b) for b in range(B)]
    pnp = lambda: mvg.ceresPnP_batch([q["unpx"] for q in pn], [q["wpts"] for q in pn], np.array([q["Twc0"] for q in pn]), 10, 5.9915,
                                     True, False, np.array([q["K"] for q in pn]))
    assert pnp()[0].all()
    print(f"B = {B}: {N_CORR} correspondences, {N_KP} keypoints x {N_CAND} local-map points per pair, {10 * NRANSAC_ITER} draws "
          f"(mean inliers after P3P {np.mean([m.sum() for m in inl]):.0f}, counted draws {r['info'][:, 0].mean():.0f})", flush=True)
    tot_w = tot_k = 0.0
    for name, call in (("P3P RANSAC", p3p), ("refinement", refine), ("local-map match", match), ("computePnP", pnp)):
        wall, ktot, kt = timed(call)
        tot_w, tot_k = tot_w + wall, tot_k + ktot
        print(f"  {name:16s} wall {wall:8.3f} ms   kernels {ktot:8.3f} ms   {kt}", flush=True)
    print(f"  {'four stages':16s} wall {tot_w:8.3f} ms   kernels {tot_k:8.3f} ms", flush=True)
