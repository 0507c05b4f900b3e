#!/usr/bin/env python3
"""times ov2_relpose_refine_batch_dev (two-view pose refinement, one workgroup per frame) with hipEvents after warm-up, and in
the same job ov2_pnp_solve_batch_dev (its sibling: same structure, 28 sums per pass instead of 21) at the same shapes and
iteration limit (GPU box).  Prints kernel time, LM iterations and time per LM iteration of the slowest frame."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe, synth_ba, synth_epi
from ov2slam_amd.multi_view_geometry import MultiViewGeometry

MAX_ITERS, REPS = 10, 20
ctx = fe.Context(0)
mvg = MultiViewGeometry(ctx)
d = ctx.to_device


def timed(reset, launch):
    """min / median over REPS of the hipEvent time of launch(), reset() (restores the in/out poses) outside the bracket"""
    for _ in range(3):
        reset(); launch()
    ctx.synchronize()
    ts = []
    for _ in range(REPS):
        reset()
        ctx.timer_start()
        launch()
        ts.append(ctx.timer_stop())
    return min(ts), float(np.median(ts))


def start_of(s, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    dR, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), np.deg2rad(1.0) * a / np.linalg.norm(a)]))
    p = np.cross(s["t"], rng.normal(size=3))
    t0 = np.cos(np.deg2rad(5.0)) * s["t"] + np.sin(np.deg2rad(5.0)) * p / np.linalg.norm(p)
    return (dR @ s["R"]).reshape(9), t0 / np.linalg.norm(t0)


def relpose(B, n):
    sc = [synth_epi.make_scene(n, seed=500 + b, noise_px=0.5, outlier_frac=0.0) for b in range(B)]
    st = [start_of(s, b) for b, s in enumerate(sc)]
    off = (n * np.arange(B + 1)).astype(np.int32)
    R0, t0 = d(np.array([x[0] for x in st])), d(np.array([x[1] for x in st]))
    d_R, d_t = ctx.empty((B, 9), np.float64), ctx.empty((B, 3), np.float64)
    d_off, d_f1, d_f2 = d(off), d(np.concatenate([s["bv_kf"] for s in sc])), d(np.concatenate([s["bv_cur"] for s in sc]))
    d_K, d_st = d(np.array([s["K"] for s in sc])), ctx.empty(B, np.int32)
    d_info, d_cost = ctx.empty((B, 2), np.int32), ctx.empty((B, 2), np.float64)

    def reset():
        ctx.lib.ov2_memcpy_d2d(ctx.h, d_R.ptr, R0.ptr, R0.nbytes)
        ctx.lib.ov2_memcpy_d2d(ctx.h, d_t.ptr, t0.ptr, t0.nbytes)

    def launch():
        mvg.refine5pt_batch_dev(B, d_off, d_f1, d_f2, None, d_K, MAX_ITERS, None, d_R, d_t, d_st, d_info, d_cost)

    tmin, tmed = timed(reset, launch)
    return tmin, tmed, d_info.get()[:, 0]


def pnp(B, n):
    fr = [synth_ba.make_pnp(n, seed=3 * b + 1) for b in range(B)]
    off = (n * np.arange(B + 1)).astype(np.int32)
    T0 = d(np.stack([p["Twc0"] for p in fr]))
    d_T = ctx.empty((B, 7), np.float64)
    d_off, d_un, d_wp = d(off), d(np.concatenate([p["unpx"] for p in fr])), d(np.concatenate([p["wpts"] for p in fr]))
    d_K = d(np.stack([p["K"] for p in fr]))
    d_out, d_rem = ctx.empty(B * n, np.uint8), ctx.empty(B * n, np.uint8)
    d_ok, d_it = ctx.empty(B, np.int32), ctx.empty((B, 2), np.int32)

    def reset():
        ctx.lib.ov2_memcpy_d2d(ctx.h, d_T.ptr, T0.ptr, T0.nbytes)

    def launch():   # the robust solve alone (no L2 re-solve): one minimisation per frame, as the refinement
        mvg.ceresPnP_batch_dev(B, d_off, d_un, d_wp, None, d_K, d_T, MAX_ITERS, 5.9915, True, False, d_out, d_rem, d_ok, d_it)

    tmin, tmed = timed(reset, launch)
    return tmin, tmed, d_it.get()[:, 0]


for B, n in [(64, 2048), (64, 300), (1, 300)]:
    for name, f in (("relpose_kernel", relpose), ("pnp_kernel", pnp)):
        tmin, tmed, it = f(B, n)
        print(f"{name}: B={B} n={n}: {tmin * 1e3:.1f} us min, {tmed * 1e3:.1f} us median, LM iterations max {it.max()} mean "
              f"{it.mean():.1f}, {tmin * 1e3 / max(int(it.max()), 1):.1f} us per LM iteration of the slowest frame", flush=True)
