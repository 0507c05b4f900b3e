#!/usr/bin/env python3
"""ov2_map_triangulate_temporal_batch: device time per call (hipEvent around the asynchronous form) for B = 1 and 64 map
mirrors of bench size (50 keyframes / 10 k landmarks) and EuRoC size (20 keyframes / 2 k landmarks), and its launch
count -- GPU box.  Every timed call starts from the same saved state (ov2_map_restore_state_batch, not timed)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, synth_temporal

ctx = fe.Context(0)
for name, n_kf, n_lm in (("bench", 50, 10000), ("euroc", 20, 2000)):
    m = synth_temporal.make_map(n_kf, n_lm, seed=1, dangling=False)
    for B in (1, 64):
        maps = [DM.DeviceMap.from_temporal_map(ctx, m) for _ in range(B)]
        for x in maps:
            x.save_state()
        call = lambda lists=False: DM.triangulate_temporal_batch(ctx, maps, calib_l=m["K4"], stereo=True, max_reproj_err=3.0, want_lists=lists)
        out = call(True)[0]
        ms = []
        for _ in range(23):
            DM.restore_state_batch(ctx, maps)
            ctx.synchronize()
            ctx.timer_start()
            call()
            ms.append(ctx.timer_stop())
        DM.restore_state_batch(ctx, maps)
        ctx.synchronize()
        ctx.kernel_timing(True); ctx.kernel_times()
        call()
        kt = ctx.kernel_times(); ctx.kernel_timing(False)
        launches = sum(v[1] for v in kt.values())
        us = float(np.median(ms[3:])) * 1e3
        rows = len(m["obs_kf"])
        print(f"{name} size ({n_kf} KF / {n_lm} landmarks / {rows} observation rows), B = {B}: {us:.1f} us per call "
              f"({us / B:.2f} us per map), {launches} launches; per map {out['selected']} 2D keypoints, {out['candidates']} candidates, "
              f"{len(out['good_lmid'])} good, {len(out['removed_lmid'])} removed", flush=True)
        for x in maps:
            x.close()
