#!/usr/bin/env python3
"""ov2_map_filter_keyframes_batch: time per call for B = 1 and 64 map mirrors of bench size (50 keyframes / 10 k landmarks)
and of the largest test size (40 keyframes / 1200 landmarks), its launch count, and the C++ host stage
(Estimator::mapFiltering on the Frame / MapPoint graph) on the same maps -- GPU box.  The call synchronises once, for the
headers and the removed lists, so it is timed on the host clock around the call; every timed call starts from the same saved
state (ov2_map_restore_state_batch + a synchronisation, not timed).  The host stage edits its map, so each of its repetitions
gets a fresh map (the construction is not timed)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_filter

ctx = fe.Context(0)
RATIO = 0.9
for name, n_kf, n_lm in (("bench", 50, 10000), ("test", 40, 1200)):
    m = synth_filter.make_map(n_kf, n_lm, seed=1)
    rows = len(m["obs_kf"])
    host_us = []
    for _ in range(5):
        hm = host_map.FilterMap(m)
        t0 = time.perf_counter()
        removed, st = hm.map_filtering(ratio=RATIO)
        host_us.append((time.perf_counter() - t0) * 1e6)
        del hm
    print(f"{name} size ({n_kf} KF / {n_lm} landmarks / {rows} observation rows): host stage {np.median(host_us):.1f} us per map "
          f"({st['candidates']} candidates, {len(removed)} removed)", flush=True)
    for B in (1, 64):
        maps = [DM.DeviceMap.from_filter_map(ctx, m) for _ in range(B)]
        for x in maps:
            x.save_state()
        out = DM.filter_keyframes_batch(ctx, maps, ratio=RATIO)[0]
        assert out["removed"] == removed
        us = []
        for _ in range(23):
            DM.restore_state_batch(ctx, maps)
            ctx.synchronize()
            t0 = time.perf_counter()
            DM.filter_keyframes_batch(ctx, maps, ratio=RATIO)
            us.append((time.perf_counter() - t0) * 1e6)
        DM.restore_state_batch(ctx, maps)
        ctx.synchronize()
        ctx.kernel_timing(True); ctx.kernel_times()
        DM.filter_keyframes_batch(ctx, maps, ratio=RATIO)
        kt = ctx.kernel_times(); ctx.kernel_timing(False)
        launches = sum(v[1] for v in kt.values())
        dev_us = sum(v[0] for v in kt.values()) * 1e3
        t = float(np.median(us[3:]))
        print(f"{name} size, B = {B}: {t:.1f} us per call on the host clock, Python wrapper and list copies included ({t / B:.2f} us per map), "
              f"{launches} launches, {dev_us:.1f} us of kernel time; per map {out['candidates']} candidates, {len(out['removed'])} removed, "
              f"{len(out['unset3d'])} landmarks lost is3d_", flush=True)
        for x in maps:
            x.close()
