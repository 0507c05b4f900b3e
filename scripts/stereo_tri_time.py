#!/usr/bin/env python3
"""ov2_map_triangulate_stereo_batch and ov2_map_set_obs_stereo_batch_dev on 64 map mirrors of EuRoC size (20 keyframes / 2500
landmarks, about 300 stereo keypoints without a 3D point in the new keyframe) -- GPU box.  Wall time (host clock around calls
that end in a stream synchronise) and device time (events around the asynchronous form), medians of 20 after 3 warm-up runs:
  1. one batched call against the same work as 64 single calls;
  2. one batched call against 64 calls of the host stage on attached maps, each with the flush that carries its edits to the
     mirror -- the path a mirror-only map had to take before;
  3. the chain intake -> stage against Frame::updateKeypointStereo + host stage + flush per map (ov2_map_set_obs_stereo, the
     ov2_triangulate_pairs round trip, ov2_map_set_landmarks).
Every timed device run starts from the same saved state (ov2_map_restore_state_batch, not timed); a host map is used once."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_stereo_tri as SST

B, WARM, REPS = 64, 3, 20
ctx = fe.Context(0)
m = SST.make_map(20, 2500, seed=1, rectified=False, new_frac=0.2)
new = m["obs_kf"] == m["newkf"]
m0 = dict(m, obs_stereo=np.where(new, 0, m["obs_stereo"]).astype(np.uint8))       # the new keyframe before its stereo matching
sel = new & (m["obs_stereo"] != 0)
lm, rxy = m["obs_lm"][sel], m["obs_rpx"][sel]
rig = DM.StereoRigC.of(m)


def timed(run, reset):
    """(median wall ms, median device ms) of run() from the state reset() leaves"""
    wall, dev = [], []
    for i in range(WARM + REPS):
        reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        run()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        reset()
        ctx.synchronize()
        ctx.timer_start()
        run()
        dev.append(ctx.timer_stop())
    return float(np.median(wall[WARM:])), float(np.median(dev[WARM:]))


# 1. batched against single calls, on maps that carry their stereo flags
maps = [DM.DeviceMap.from_stereo_tri_map(ctx, m) for _ in range(B)]
for x in maps:
    x.save_state()
reset = lambda: DM.restore_state_batch(ctx, maps)
out = DM.triangulate_stereo_batch(ctx, maps[:1], rigs=rig)[0]
reset()
bw, bd = timed(lambda: DM.triangulate_stereo_batch(ctx, maps, rigs=rig, want_lists=False), reset)
sw, sd = timed(lambda: [DM.triangulate_stereo_batch(ctx, [x], rigs=rig, want_lists=False) for x in maps], reset)
print(f"{B} maps of {m['n_kf']} KF / {m['n_lm']} landmarks / {len(m['obs_kf'])} rows; per map {out['selected']} stereo 2D keypoints, "
      f"{len(out['good_lmid'])} good, {len(out['demoted_lmid'])} demoted", flush=True)
print(f"1. stage, one call of B = {B}: wall {bw:.3f} ms, device {bd:.3f} ms; {B} calls of B = 1: wall {sw:.3f} ms, device {sd:.3f} ms", flush=True)

# 3a. the chain on the device: verdicts onto the rows, then the stage, no host round trip between them
for x in maps:
    x.close()
maps = [DM.DeviceMap.from_stereo_tri_map(ctx, m0) for _ in range(B)]
for x in maps:
    x.save_state()
d_lm, d_st, d_rxy = ctx.to_device(lm), ctx.to_device(np.ones(len(lm), np.uint8)), ctx.to_device(rxy)
kf = [m["newkf"]] * B


def chain():
    DM.set_obs_stereo_batch_dev(ctx, maps, kf, [d_lm] * B, [d_st] * B, [d_rxy] * B)
    DM.triangulate_stereo_batch(ctx, maps, rigs=rig, want_lists=False)


cw, cd = timed(chain, reset)
print(f"3. chain intake -> stage, B = {B}: wall {cw:.3f} ms, device {cd:.3f} ms", flush=True)
for x in maps:
    x.close()

# 2. / 3b. the host paths, one fresh attached map per sample
h2, h3 = [], []
for i in range(WARM + REPS):
    hm = host_map.StereoTriMap(m)
    hm.attach_device(ctx)
    ctx.synchronize()
    t0 = time.perf_counter()
    hm.triangulate_stereo(ctx, 3.0)
    hm.flush_device()
    h2.append((time.perf_counter() - t0) * 1e3)
    hm = host_map.StereoTriMap(m0)
    hm.attach_device(ctx)
    ctx.synchronize()
    t0 = time.perf_counter()
    hm.set_kp_stereo(m["newkf"], lm, rxy)
    hm.triangulate_stereo(ctx, 3.0)
    hm.flush_device()
    h3.append((time.perf_counter() - t0) * 1e3)
p2, p3 = float(np.median(h2[WARM:])), float(np.median(h3[WARM:]))
print(f"2. host stage + flush on an attached map: wall {p2:.3f} ms per map, {B * p2:.2f} ms for {B} maps "
      f"(batched device call: {bw:.3f} ms, x{B * p2 / bw:.0f})", flush=True)
print(f"3. updateKeypointStereo + host stage + flush: wall {p3:.3f} ms per map, {B * p3:.2f} ms for {B} maps "
      f"(device chain: {cw:.3f} ms, x{B * p3 / cw:.0f})", flush=True)
