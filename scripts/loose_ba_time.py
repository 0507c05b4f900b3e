#!/usr/bin/env python3
"""ov2_map_loose_ba_batch: time for 64 map mirrors of a make_window(20, 2500) sized map (inverse depth, EuRoC-sized), the
range being the ten newest keyframes below the newest three (keyframes 7..16 of 20) -- GPU box.  Reported: one batched call
(wall), 64 single-map calls of the same entry point (wall), 64 calls of the host stage Optimizer::looseBA on host maps with a
mirror attached (HostMap.loose_ba: hash-map walk, flat problem, the same solver through its host form, write-back; the flush
of the mirror is not timed), and the device time of the three stages of one batched call (set-up chain, solve, update), each
the sum of its kernels' event times.  The 64 maps hold the same window (building 64 distinct ones costs more than the
measurement); every mirror is rewound between repetitions (ov2_map_restore_state_batch, not timed), every host map is built
fresh for its one timed call (construction not timed; one call on a spare map warms the solver up).  Wall time is the host
clock around the call, Python wrapper included (records only: the replay lists stay on the device); the median of REPS
repetitions is reported."""
import sys, os, time
import ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_ba

ctx = fe.Context(0)
B, REPS = 64, 5
INI, N = 7, 16
P0 = synth_ba.make_window(20, 2500, inv_depth=True, outlier_frac=0.08)
P0.res_uv = P0.res_uv.astype(np.float32).astype(np.float64)   # keypoints are cv::Point2f in the map
P0.lm_anchor_uv = P0.lm_anchor_uv.astype(np.float32).astype(np.float64)
cam = DM.SbaCamC.of(P0)
print(f"map: {len(P0.pose)} keyframes, {len(P0.lm)} landmarks, {P0.n_res} residual blocks; range [{INI}, {N}]", flush=True)


def median_us(prepare, call):
    us = []
    for _ in range(REPS):
        prepare()
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us))


def kernel_us(call):
    ctx.synchronize()
    ctx.kernel_timing(True); ctx.kernel_times()
    out = call()
    kt = ctx.kernel_times(); ctx.kernel_timing(False)
    return out, sum(v[0] for v in kt.values()) * 1e3, sum(v[1] for v in kt.values())


spare = host_map.HostMap(P0)
spare.loose_ba(ctx, INI, N)
del spare
maps = [DM.DeviceMap.from_problem(ctx, P0, isobs="newest") for _ in range(B)]
for m in maps:
    m.save_state()
rewind = lambda: DM.restore_state_batch(ctx, maps)
lo, hi, cams = [INI] * B, [N] * B, [cam] * B
batched = median_us(rewind, lambda: DM.loose_ba_batch(ctx, maps, lo, hi, cams, cur_kfid=[N] * B, fetch_lists=False))
singles = median_us(rewind, lambda: [DM.loose_ba_batch(ctx, [m], [INI], [N], [cam], cur_kfid=[N], fetch_lists=False) for m in maps])
# the three stages of one batched call, each under the kernel timer
rewind()
views, setup_us, setup_n = kernel_us(lambda: DM.loose_setup_batch(ctx, maps, lo, hi, 1, True, P0.calib_l))
pcs, rcs = DM.problems_of(views, P0, True)
o = DM.loose_ba_options(ctx)
st, solve_us, solve_n = kernel_us(lambda: ctx.lib.ov2_ba_solve_batch_dev(ctx.h, B, pcs, C.byref(o), rcs))
assert st == 0
recs, update_us, update_n = kernel_us(lambda: DM.loose_update_batch(ctx, maps, views, cur_kfid=[N] * B))
res = float(np.mean([r["n_res"] for r in recs]))
host_us, host_n1 = [], []
for b in range(B):
    hm = host_map.HostMap(P0)
    hm.attach_device(ctx)
    hm.set_cur_frame(N)
    ctx.synchronize()
    t0 = time.perf_counter()
    st, n1, fc = hm.loose_ba(ctx, INI, N)
    host_us.append((time.perf_counter() - t0) * 1e6)
    host_n1.append(n1)
    del hm
for m in maps:
    m.close()
print(f"looseBA of {B} maps ({res:.0f} residual blocks, {recs[0]['n_pose']} poses of which {recs[0]['n_free_pose']} free, "
      f"{recs[0]['n_lm']} landmarks per map; {recs[0]['n_flagged_left'] + recs[0]['n_flagged_right']} flagged blocks, host {host_n1[0]}): "
      f"one batched call {batched:.1f} us wall ({batched / B:.1f} us per map); {B} single-map calls {singles:.1f} us wall; "
      f"{B} host-stage calls {sum(host_us):.1f} us wall (median {np.median(host_us):.1f} us per map); device time of one batched "
      f"call by stage: set-up chain {setup_us:.1f} us in {setup_n} launches, solve {solve_us:.1f} us in {solve_n} launches, "
      f"update {update_us:.1f} us in {update_n} launches", flush=True)
