#!/usr/bin/env python3
"""Optimizer::localPoseGraph on mirror-only maps, three ways -- GPU box.  B = 64 maps, a chain of 20 keyframes (maps of 24
keyframes / 2500 landmarks) and a chain of 200 keyframes (maps of 204 keyframes / 2500 landmarks); the loop keyframe is 1, the
new keyframe nk - 4, newTwc the stored pose times a twist of norm 0.05.
1. ov2_map_local_pose_graph_batch with out == NULL, ended by one stream synchronisation.
2. what a mirror-only caller had before that entry point: ov2_map_download of the poses of every map, the chain and its
   edges assembled on the host (numpy stand-in for Optimizer::assembleLocalPoseGraph), ov2_pose_graph_solve_batch (upload,
   launch, download, synchronisation), the degenerate test on the host, ov2_map_pose_graph_update_batch (no header) and a
   synchronisation.
3. 64 single calls of the new entry point, one synchronisation at the end.
Host clock around each variant, Python wrappers included; every timed run starts from the same saved state (restore +
synchronisation, not timed); median of 10 after 2 warm-up runs.  Launch counts and device time per launch come from the
context's kernel counters in a run of their own."""
import sys, os, time
import ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from scipy.linalg import expm
from ov2slam_amd import ba_types as T, device_map as DM, frontend as fe, pose_graph, synth_filter
from test_oracle_pg import hat6, mat, pose7

ctx = fe.Context(0)
B, LOOP = 64, 1


def qmul(a, b):
    x1, y1, z1, w1 = a.T
    x2, y2, z2, w2 = b.T
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], 1)


def qrot(q, v):
    u, w = q[:, :3], q[:, 3:]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def rel(Ti, Tj):
    """inverse(Ti) * Tj on (n, 7) arrays"""
    qi = Ti[:, 3:] * np.array([-1, -1, -1, 1.0])
    return np.hstack([qrot(qi, Tj[:, :3] - Ti[:, :3]), qmul(qi, Tj[:, 3:])])


def host_path(maps, newkf, Tn):
    """variant 2; returns the verdicts"""
    probs, chains = [], []
    for m in maps:
        nk = C.c_int()
        ctx.lib.ov2_map_download(m.h, C.byref(nk), None, None, *([None] * 9))
        pose, state = np.zeros((nk.value, 7)), np.zeros(nk.value, np.uint8)
        ctx.lib.ov2_map_download(m.h, None, None, None, pose.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p), *([None] * 7))
        ids = np.flatnonzero(state[:newkf + 1])
        ids = ids[ids >= LOOP].astype(np.int32)
        P = pose[ids]
        n = len(ids)
        Tij = np.vstack([rel(P[:-1], P[1:]), rel(P[:1], Tn[None])])
        cst = np.zeros(n, np.uint8); cst[0] = 1
        probs.append(T.PgProblem(P, cst, np.append(np.arange(n - 1), 0), np.append(np.arange(1, n), n - 1), Tij))
        chains.append(ids)
    pose_graph.solve_batch(ctx, probs)
    ok = [np.linalg.norm(Tn[:3] - p.pose[-1, :3]) <= 0.3 for p in probs]
    DM.pose_graph_update_batch(ctx, maps, [newkf] * len(maps), [c[1:] if k else c[:0] for c, k in zip(chains, ok)],
                               [p.pose[1:] if k else p.pose[:0] for p, k in zip(probs, ok)], want_header=False)
    ctx.synchronize()
    return ok


def timed(fn, maps, reps=12, warm=2):
    us = []
    for _ in range(reps):
        DM.restore_state_batch(ctx, maps)
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us[warm:]))


def counters(fn, maps):
    DM.restore_state_batch(ctx, maps)
    ctx.synchronize()
    ctx.kernel_timing(True); ctx.kernel_times()
    fn()
    kt = ctx.kernel_times(); ctx.kernel_timing(False)
    return ", ".join(f"{n} {c} x {ms * 1e3 / c:.1f} us" for n, (ms, c) in sorted(kt.items()))


for nk, nl in ((24, 2500), (204, 2500)):
    m = synth_filter.make_map(nk, nl, seed=1)
    newkf = nk - 4
    v = np.random.default_rng(5).normal(0, 1, 6)
    Tn = pose7(mat(m["poses"][newkf]) @ expm(hat6(v / np.linalg.norm(v) * 0.05)))
    maps = [DM.DeviceMap.from_filter_map(ctx, m) for _ in range(B)]
    for x in maps:
        x.save_state()
    nks, los, Ts = [newkf] * B, [LOOP] * B, [Tn] * B

    def new_call():
        DM.local_pose_graph_batch(ctx, maps, nks, los, Ts, want=False)
        ctx.synchronize()

    def old_path():
        host_path(maps, newkf, Tn)

    def singles():
        for x in maps:
            DM.local_pose_graph_batch(ctx, [x], [newkf], [LOOP], [Tn], want=False)
        ctx.synchronize()

    DM.restore_state_batch(ctx, maps); ctx.synchronize()
    r = DM.local_pose_graph_batch(ctx, maps, nks, los, Ts)[0]
    t1, t2, t3 = timed(new_call, maps), timed(old_path, maps), timed(singles, maps)
    print(f"{B} maps of {nk} KF / {nl} landmarks / {len(m['obs_kf'])} rows, chain of {r['n_pose']} poses, {r['result'].n_log} log entries, "
          f"verdict {r['verdict']}:", flush=True)
    print(f"  1. one ov2_map_local_pose_graph_batch call + synchronise: {t1:.0f} us ({t1 / B:.1f} us per map)", flush=True)
    print(f"     launches: {counters(new_call, maps)}", flush=True)
    print(f"  2. download + host assembly + ov2_pose_graph_solve_batch + host gate + ov2_map_pose_graph_update_batch: {t2:.0f} us "
          f"({t2 / B:.1f} us per map), ratio {t2 / t1:.2f}", flush=True)
    print(f"     launches: {counters(old_path, maps)}", flush=True)
    print(f"  3. {B} single calls + one synchronise: {t3:.0f} us ({t3 / B:.1f} us per map), ratio {t3 / t1:.2f}", flush=True)
    for x in maps:
        x.close()
