#!/usr/bin/env python3
"""ov2_map_structure_ba_batch: time for 64 map mirrors of a make_window(20, 2500) sized map (XYZ points), each with a list of
12 points (what one matchToMap round merges) and of 100 points (a loop's merged points) -- GPU box.  Four numbers per list
length: one batched call (wall), the device time of its solver launch, 64 single-map calls (wall), and the path a map had
before the mirror form existed: Optimizer::structureOnlyBA of the C++ host mirror per map (HostMap.structure_only_ba: host
walk, flat problem, the general local-BA solver, write-back) on the SAME 64 problems.  Every map starts from its own seeded
noise (0.1 m) on the listed points; the mirrors are rewound between repetitions (ov2_map_restore_state_batch, not timed), the
host maps are built fresh for their one timed call each (construction not timed; one call on a spare map warms the solver
up).  Wall time is the host clock around the call, Python wrapper included (a call synchronises once, for the records);
the median of REPS repetitions is reported."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_ba

ctx = fe.Context(0)
B, REPS = 64, 5
P0 = synth_ba.make_window(20, 2500, inv_depth=False)
P0.res_uv = P0.res_uv.astype(np.float32).astype(np.float64)   # keypoints are cv::Point2f in the map
cam = DM.SbaCamC.of(P0)
print(f"map: {len(P0.pose)} keyframes, {len(P0.lm)} landmarks, {P0.n_res} residual blocks", flush=True)


def problems(n_pts):
    """the same window B times, map b with its own list of n_pts ids and its own noise on them"""
    out = []
    for b in range(B):
        rng = np.random.default_rng(1000 + b)
        ids = np.sort(rng.choice(len(P0.lm), n_pts, replace=False)).astype(np.int32)
        P = P0.copy()
        P.lm[ids] += rng.normal(0, 0.1, (n_pts, 3))
        out.append((P, ids))
    return out


def median_us(prepare, call):
    us = []
    for _ in range(REPS):
        prepare()
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us))


spare = host_map.HostMap(P0)
spare.structure_only_ba(ctx, np.arange(12, dtype=np.int32))
del spare
for n_pts in (12, 100):
    probs = problems(n_pts)
    maps = [DM.DeviceMap.from_problem(ctx, P) for P, _ in probs]
    lists, cams = [ids for _, ids in probs], [cam] * B
    for m in maps:
        m.save_state()
    rewind = lambda: DM.restore_state_batch(ctx, maps)
    batched = median_us(rewind, lambda: DM.structure_ba_batch(ctx, maps, lists, cams))
    singles = median_us(rewind, lambda: [DM.structure_ba_batch(ctx, [m], [l], [cam]) for m, l in zip(maps, lists)])
    rewind(); ctx.synchronize()
    ctx.kernel_timing(True); ctx.kernel_times()
    hdr = DM.structure_ba_batch(ctx, maps, lists, cams)
    kt = ctx.kernel_times(); ctx.kernel_timing(False)
    launches, solver_us = sum(v[1] for v in kt.values()), kt["map_sba_kernel"][0] * 1e3
    chain_us = sum(v[0] for v in kt.values()) * 1e3
    evals = float(np.mean([h["n_log"] for h in hdr]))   # row passes of a map: iteration zero + one per logged step
    res = float(np.mean([h["n_res"] for h in hdr]))
    host_us, host_cost = [], []
    for P, ids in probs:
        hm = host_map.HostMap(P)
        ctx.synchronize()
        t0 = time.perf_counter()
        st, cost, its = hm.structure_only_ba(ctx, ids)
        host_us.append((time.perf_counter() - t0) * 1e6)
        host_cost.append(cost)
        del hm
    worst = max(abs(h["final_cost"] / c - 1) for h, c in zip(hdr, host_cost))
    for m in maps:
        m.close()
    print(f"{n_pts} listed points per map ({res:.0f} residual blocks, {evals:.1f} row passes on average): one batched call of {B} "
          f"{batched:.1f} us wall ({batched / B:.2f} us per map); its solver launch {solver_us:.1f} us of device time "
          f"({solver_us / evals:.1f} us per row pass), {launches} launches, {chain_us:.1f} us of kernel time in all; {B} single-map calls "
          f"{singles:.1f} us wall; {B} host-stage calls {sum(host_us):.1f} us wall (median {np.median(host_us):.1f} us per map); "
          f"final costs agree to {worst:.1e}", flush=True)
