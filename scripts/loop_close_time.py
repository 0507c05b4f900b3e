#!/usr/bin/env python3
"""The two device pieces behind an accepted loop, batched -- GPU box.
1. ov2_pose_graph_solve_batch: 64 loop-closed chains of 50 keyframes through ONE call against 64 ov2_pose_graph_solve calls
   (hipEvent pair around the calls: staging upload, launch(es), download, synchronisation(s)).  Every timed run starts from
   fresh copies of the same problems; median of 20 after 3 warm-up runs.
2. ov2_map_pose_graph_update_batch: B = 1 and 64 map mirrors of bench size (50 keyframes / 10 k landmarks, the size
   scripts/filter_time.py uses), chain = keyframes 5 .. 46 with perturbed poses, header asked for (one synchronisation), timed
   on the host clock around the call; every timed call starts from the same saved state (restore + synchronisation, not
   timed).  Its launch count and kernel time come from the context's kernel counters."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from scipy.linalg import expm
from ov2slam_amd import device_map as DM, frontend as fe, pose_graph, synth_filter
from test_oracle_pg import chain, hat6, mat, pose7

ctx = fe.Context(0)

B, n = 64, 50
P0 = [chain(np.random.default_rng(1000 + b), n, drift=0.01)[0] for b in range(B)]
one, many = [], []
for _ in range(23):
    Ps = [P.copy() for P in P0]
    ctx.synchronize()
    ctx.timer_start()
    Rs = pose_graph.solve_batch(ctx, Ps)
    many.append(ctx.timer_stop())
    Qs = [P.copy() for P in P0]
    ctx.synchronize()
    ctx.timer_start()
    Rq = [pose_graph.solve(ctx, Q) for Q in Qs]
    one.append(ctx.timer_stop())
assert all(np.array_equal(P.pose, Q.pose) for P, Q in zip(Ps, Qs))
tb, ts = float(np.median(many[3:])) * 1e3, float(np.median(one[3:])) * 1e3
print(f"{B} chains of {n} keyframes / {len(P0[0].edge_i)} edges, {np.mean([R.n_log for R in Rs]):.1f} log entries each: one batch call "
      f"{tb:.1f} us ({tb / B:.1f} us per graph), {B} single calls {ts:.1f} us ({ts / B:.1f} us per graph), ratio {ts / tb:.1f}", flush=True)

n_kf, n_lm = 50, 10000
m = synth_filter.make_map(n_kf, n_lm, seed=1)
newkf = n_kf - 4
ids = np.arange(5, newkf + 1, dtype=np.int32)
rng = np.random.default_rng(1)
T = np.stack([pose7(mat(m["poses"][k]) @ expm(hat6(rng.normal(0, 0.01, 6)))) for k in ids])
for B in (1, 64):
    maps = [DM.DeviceMap.from_filter_map(ctx, m) for _ in range(B)]
    for x in maps:
        x.save_state()
    args = dict(newkf=[newkf] * B, chain_kfid=[ids] * B, chain_Twc=[T] * B)
    us = []
    for _ in range(23):
        DM.restore_state_batch(ctx, maps)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = DM.pose_graph_update_batch(ctx, maps, **args)
        us.append((time.perf_counter() - t0) * 1e6)
    DM.restore_state_batch(ctx, maps)
    ctx.synchronize()
    ctx.kernel_timing(True); ctx.kernel_times()
    DM.pose_graph_update_batch(ctx, maps, **args)
    kt = ctx.kernel_times(); ctx.kernel_timing(False)
    launches, dev_us = sum(v[1] for v in kt.values()), sum(v[0] for v in kt.values()) * 1e3
    t = float(np.median(us[3:]))
    print(f"mirror update, {n_kf} KF / {n_lm} landmarks / {len(m['obs_kf'])} rows, B = {B}: {t:.1f} us per call on the host clock, Python "
          f"wrapper included ({t / B:.2f} us per map), {launches} launches, {dev_us:.1f} us of kernel time; per map "
          f"{out[0]['n_kf_chain']} chain + {out[0]['n_kf_younger']} younger keyframes, {out[0]['n_lm_moved']} landmarks moved", flush=True)
    for x in maps:
        x.close()
