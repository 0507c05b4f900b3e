#!/usr/bin/env python3
"""ov2_map_merge_points_batch: time per call for B = 1 and 64 map mirrors of the largest test size (40 keyframes / 1200
landmarks) and of a EuRoC-sized map (50 keyframes / 10 k landmarks), each map with a matchToMap-sized list (12 pairs) and a
loop-sized list (300 pairs) -- GPU box.  One batched call is compared with B single-map calls, and with the same merges
through a host MapManager with the mirror attached (mergeMapPoints x n, then flushDevice).  A merge edits the map and a map
with a saved state is refused, so every timed call gets fresh mirrors (their construction is not timed): few repetitions,
the median is reported.  Wall time is the host clock around the call, Python wrapper included (the call synchronises once,
for headers and statuses); device time is the sum of the context's kernel timers over one more call."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_filter

ctx = fe.Context(0)
REPS = 3
L = host_map.lib()
L.ov2h_map_merge_points.argtypes = [C.c_void_p, C.c_int, C.c_int]


def pair_list(m, n, seed):
    """n random pairs of observed 3D landmarks, prev != new"""
    rng = np.random.default_rng(seed)
    ids = np.intersect1d(np.flatnonzero(m["lm_3d"]), m["obs_lm"])
    p = rng.choice(ids, (n, 2))
    return p[p[:, 0] != p[:, 1]].astype(np.int32)


def timed(maps_of, call):
    us = []
    for _ in range(REPS):
        maps = maps_of()
        ctx.synchronize()
        t0 = time.perf_counter()
        call(maps)
        us.append((time.perf_counter() - t0) * 1e6)
        for x in maps:
            x.close()
    return float(np.median(us))


for name, n_kf, n_lm in (("test", 40, 1200), ("EuRoC", 50, 10000)):
    m = synth_filter.make_map(n_kf, n_lm, seed=1)
    rows = len(m["obs_kf"])
    for what, n_pairs in (("matchToMap", 12), ("loop", 300)):
        pairs = pair_list(m, n_pairs, seed=n_pairs)
        host_us = []
        for _ in range(REPS):
            hm = host_map.FilterMap(m)
            hm.attach_device(ctx)
            ctx.synchronize()
            t0 = time.perf_counter()
            for p, n in pairs.tolist():
                L.ov2h_map_merge_points(hm.h, p, n)
            hm.flush_device()
            ctx.synchronize()
            host_us.append((time.perf_counter() - t0) * 1e6)
            del hm
        print(f"{name} size ({n_kf} KF / {n_lm} landmarks / {rows} rows), {what} list of {len(pairs)} pairs: host MapManager with the "
              f"mirror attached {np.median(host_us):.1f} us per map (mergeMapPoints x n + flushDevice)", flush=True)
        for B in (1, 64):
            fresh = lambda: [DM.DeviceMap.from_filter_map(ctx, m) for _ in range(B)]
            batched = timed(fresh, lambda maps: DM.merge_points_batch(ctx, maps, [pairs] * B))
            singles = timed(fresh, lambda maps: [DM.merge_points_batch(ctx, [x], [pairs]) for x in maps])
            maps = fresh()
            ctx.synchronize()
            ctx.kernel_timing(True); ctx.kernel_times()
            hdr, _ = DM.merge_points_batch(ctx, maps, [pairs] * B)
            kt = ctx.kernel_times(); ctx.kernel_timing(False)
            for x in maps:
                x.close()
            launches, dev_us = sum(v[1] for v in kt.values()), sum(v[0] for v in kt.values()) * 1e3
            h = hdr[0]
            print(f"  B = {B}: one batched call {batched:.1f} us wall ({batched / B:.2f} us per map), {B} single-map calls {singles:.1f} us wall; "
                  f"{launches} launches, {dev_us:.1f} us of kernel time; per map {h['n_merged']} merged, {h['n_skipped']} skipped, "
                  f"{h['n_rows_moved']} rows moved, {h['n_rows_conflict']} in conflict", flush=True)
