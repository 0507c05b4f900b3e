#!/usr/bin/env python3
"""times ov2_knn2_hamming_batch_dev (the loop-candidate matcher alone, arrays resident in HBM) on an MI355X at
1 x (300 x 300), 1 x (2048 x 2048) and 64 x (2048 x 2048), and at 2 x and 8 x (2048 x 2048) between them, for every lane
mapping and for the automatic choice.
Device events around N back-to-back launches; the mappings alternate inside each of ROUNDS rounds, so that the spread of a
mapping over the rounds is the run-to-run noise its median is held against.  Prints the VALU floor beside each time:
distances x VALU instructions per distance of the compiled inner loop / (CUs x 4 SIMDs x 16 lanes per clock x clock)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ov2slam_amd import frontend as fe

ROUNDS = 7
LANES = (0, 1, 4, 16, 64)
VALU_PER_DISTANCE = 24       # inner loop of knn2_kernel<1> as compiled for gfx950, per distance: 8 v_xor + 8 v_bcnt + 3 v_add3 + 5 (key, min / max, address moves)
CUS, CLOCK_GHZ = 256, 2.4    # MI355X
# B, n_query, n_train, launches per window: the three sizes the stage is sized for, and two between them at which the automatic
# choice takes 16 and 4 lanes per query
SHAPES = ((1, 300, 300, 2000), (1, 2048, 2048, 400), (64, 2048, 2048, 40), (2, 2048, 2048, 400), (8, 2048, 2048, 200))

ctx = fe.Context(0)
rng = np.random.default_rng(0)


def window(B, total_q, arrays, n):
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(n):
        st = ctx.lib.ov2_knn2_hamming_batch_dev(ctx.h, B, total_q, *arrays)
        assert st == 0
    return ctx.timer_stop() / n * 1e3   # us per launch


for B, nq, nt, n in SHAPES:
    qo = (np.arange(B + 1) * nq).astype(np.int32)
    to = (np.arange(B + 1) * nt).astype(np.int32)
    dev = [ctx.to_device(a) for a in (qo, to, rng.integers(0, 256, (B * nq, 32), dtype=np.uint8),
                                      rng.integers(0, 256, (B * nt, 32), dtype=np.uint8),
                                      np.zeros((B * nq, 2), np.int32), np.zeros((B * nq, 2), np.int32))]
    arrays = [d.ptr for d in dev]
    out = {}
    for lanes in LANES:            # warm up every mapping at this shape, and check that all give the same bits
        ctx.set_knn_lanes(lanes)
        window(B, B * nq, arrays, 3)
        out[lanes] = (dev[4].get(), dev[5].get())
        assert np.array_equal(out[lanes][0], out[0][0]) and np.array_equal(out[lanes][1], out[0][1])
    t = {lanes: [] for lanes in LANES}
    for _ in range(ROUNDS):
        for lanes in LANES:
            ctx.set_knn_lanes(lanes)
            t[lanes].append(window(B, B * nq, arrays, n))
    ctx.set_knn_lanes(0)
    floor = B * nq * nt * VALU_PER_DISTANCE / (CUS * 4 * 16 * CLOCK_GHZ * 1e3)   # us
    print(f"{B} x ({nq} x {nt}): VALU floor {floor:.2f} us", flush=True)
    for lanes in LANES:
        v = np.array(t[lanes])
        med = float(np.median(v))
        print(f"  lanes {lanes:2d}: median {med:9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  floor / median {floor / med:.3f}", flush=True)
