#!/usr/bin/env python3
"""ov2_map_local_ids_batch: 64 map mirrors of 21 keyframes / 2500 landmarks in one call, the same maps as 64 single calls, and
the C++ host stage (MapManager::updateFrameCovisibility + SlamManager::extendLocalMap on the Frame / MapPoint graph) on 64
host_map.LoopMap objects of the same maps -- GPU box.  The call synchronises once, for the headers and the lists, so it is timed
on the host clock around the call, Python wrapper and list copies included.  Every timed call meets the state the call before
it left: the new keyframe's stored set is its last result (the store rule swaps it for the same S) and the oldest covisible
keyframe holds a stored set of 300 ids, so the extension branch is taken every time.  Every call replaces a set of about 1400
ids, so the pool of a map meets its squeeze rule every few calls whatever its size: the timed calls are a mix of calls with
and without a squeeze, and the script prints the fastest and the slowest call beside the median and how many squeezed."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import device_map as DM, frontend as fe, host_map, synth_filter

B, N_KF, N_LM, NMAX = 64, 21, 2500, 100000   # 21 keyframes: the smallest map synth_filter makes
ctx = fe.Context(0)
src = [synth_filter.make_map(N_KF, N_LM, seed=1 + b) for b in range(B)]
maps = [DM.DeviceMap.from_filter_map(ctx, m) for m in src]
for x in maps:
    x.enable_local_sets(4 * N_LM)
first = DM.local_ids_batch(ctx, maps, extend=False)
stored = [np.arange(N_LM, N_LM + 300, dtype=np.int32) for _ in range(B)]
for x, r, ids in zip(maps, first, stored):
    x.set_local_set(r["oldest_cov"], ids)
rows = [len(m["obs_kf"]) for m in src]
print(f"{B} maps, {N_KF} KF / {N_LM} landmarks / {min(rows)}..{max(rows)} observation rows each; per map {len(first[0]['cov_kfid'])} covisible "
      f"keyframes, |S| = {first[0]['n_fresh']}", flush=True)


def timed(fn, reps=23, skip=3):
    us = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us[skip:])), float(np.min(us[skip:])), float(np.max(us[skip:]))


batch = DM.local_ids_batch(ctx, maps, extend=True, nmax_local=NMAX)
assert all(r["extended"] and len(r["lmid"]) == r["n_fresh"] + 300 for r in batch)
sq0 = maps[0].local_pool()["squeezes"]
t_batch, lo_batch, hi_batch = timed(lambda: DM.local_ids_batch(ctx, maps, extend=True, nmax_local=NMAX))
sq_batch = maps[0].local_pool()["squeezes"] - sq0
t_single, lo_single, hi_single = timed(lambda: [DM.local_ids_batch(ctx, [x], extend=True, nmax_local=NMAX) for x in maps], reps=9, skip=2)
ctx.kernel_timing(True); ctx.kernel_times()
DM.local_ids_batch(ctx, maps, extend=True, nmax_local=NMAX)
kt = ctx.kernel_times(); ctx.kernel_timing(False)
print(f"one call, B = {B}: median {t_batch:.1f} us ({t_batch / B:.2f} us per map), fastest {lo_batch:.1f}, slowest {hi_batch:.1f}; "
      f"{sum(v[1] for v in kt.values())} launches, {sum(v[0] for v in kt.values()) * 1e3:.1f} us of kernel time; every map's pool was squeezed "
      f"in {sq_batch} of the 23 calls (a squeeze is a fresh allocation, device copies and a synchronisation per map)", flush=True)
print(f"{B} single calls: median {t_single:.1f} us ({t_single / B:.2f} us per map), fastest {lo_single:.1f}, slowest {hi_single:.1f}", flush=True)
print(f"pool of map 0 after the runs: {maps[0].local_pool()}", flush=True)


def scene_of(m):
    """the synth_filter map in the layout host_map.LoopMap builds from"""
    kps = {}
    for k in range(m["n_kf"]):
        sel = m["obs_kf"] == k
        lm = m["obs_lm"][sel].astype(np.int32)
        kps[k] = dict(lmid=lm, uv=m["obs_uv"][sel].astype(np.float32), kp3d=(m["lm_kp3d"][lm] != 0).astype(np.uint8),
                      lm3d=(m["lm_3d"][lm] != 0).astype(np.uint8), xyz=m["lm_xyz"][lm])
    return dict(K4=synth_filter.K4, w=752, h=480, kfids=list(range(m["n_kf"])), poses={k: m["poses"][k] for k in range(m["n_kf"])}, kps=kps,
                desc={}, forget_lm=[], cov=[])


L = host_map.lib()
host_us = []
for _ in range(5):
    hms = [host_map.LoopMap(scene_of(m)) for m in src]
    for hm, r, ids in zip(hms, first, stored):
        hm.set_local_ids(r["oldest_cov"], ids)
    t0 = time.perf_counter()
    for hm, m in zip(hms, src):
        L.ov2h_update_frame_covisibility(hm.h, int(m["newkf"]))
        L.ov2h_extend_local_map(hm.h, int(m["newkf"]), NMAX)
    host_us.append((time.perf_counter() - t0) * 1e6)
    got = sorted(hms[0].local_ids(int(src[0]["newkf"])))
    for hm in hms:
        hm.close()
print(f"host stage on {B} LoopMaps: {np.median(host_us):.1f} us ({np.median(host_us) / B:.2f} us per map); its set of map 0 "
      f"{'equals' if got == batch[0]['lmid'].tolist() else 'DIFFERS FROM'} the mirror's ({len(got)} ids)", flush=True)
