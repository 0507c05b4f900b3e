#!/usr/bin/env python3
"""ov2_pose_graph_solve: time per solve (hipEvent pair around the call: upload, the one pg_minimize_kernel launch that runs
the whole LM loop, download) on loop-closed chains of 40 and 200 keyframes, the sizes of tests/test_pg_gpu.py -- GPU box.
Every timed solve starts from a fresh copy of the same problem; median of 20 after 3 warm-up solves."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# chain() of tests/test_oracle_pg.py builds the problems (the same ones the GPU test solves)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from ov2slam_amd import frontend as fe, pose_graph
from test_oracle_pg import chain

ctx = fe.Context(0)
for n, drift in ((40, 0.01), (200, 0.003)):
    P0, _ = chain(np.random.default_rng(n), n, drift=drift)
    ms = []
    for _ in range(23):
        P = P0.copy()
        ctx.synchronize()
        ctx.timer_start()
        R = pose_graph.solve(ctx, P)
        ms.append(ctx.timer_stop())
    us = float(np.median(ms[3:])) * 1e3
    print(f"chain of {n} keyframes / {len(P0.edge_i)} edges: {us:.1f} us per solve, {R.n_log} LM iterations, "
          f"cost {R.initial_cost:.4g} -> {R.final_cost:.4g}", flush=True)
