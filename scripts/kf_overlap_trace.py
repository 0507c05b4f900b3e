#!/usr/bin/env python3
"""Does the keyframe detector chain really run beside the stereo matching?  Reads a `rocprofv3 --kernel-trace
--output-format csv` trace of `bench.py --no-ba` (a run of its own, no counters) and prints, per keyframe period:
  the stereo-matching interval (klt_compact_kernel .. epi_gate_kernel of the keyframe) and its klt_stage2_kernel,
  the detector-chain interval (first det_* kernel .. subpix_kernel), both relative to the start of the stereo interval,
  their overlap, the length of the period (stereo start to the next stereo start), and the summed kernel durations of
  the period by group (tracking + stereo, detector chain, pyramid builds, everything else) with the hardware queues
  each group ran on -- two groups that share a queue cannot overlap.
A second table splits the stereo interval kernel by kernel (klt_compact_kernel, the first and the second tracking launch,
epi_gate_kernel and the gaps between them) with the detector chain's interval, the period, the idle time of the tracking
kernels' queue and that of the pyramid builds' queue (over the period, and the part of it inside the stereo interval) beside
it, and closes with the mean and the lower quartile / median / upper quartile of every column.
A third table shows what follows each keyframe: the tracking queue's idle time in front of the next plain tracking call,
cornerSubPix, and the klt_stage1_kernel launch it may run beside (the lazy join of the chain, detect.hip).
usage: kf_overlap_trace.py <kernel_trace.csv or a directory holding one> [more traces ...]"""
import csv
import glob
import os
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from summarize_prof import short  # noqa: E402

DET = {"det_mask_kernel", "det_worklist_kernel", "det_mineig_kernel", "det_fast_kernel", "det_assemble_kernel", "subpix_kernel"}
KLT = {"klt_compact_kernel", "klt_stage1_kernel", "klt_stage2_kernel", "epi_gate_kernel"}
PYR = {"clahe_lut_kernel", "level0_kernel", "level_kernel", "level23_kernel", "clahe_level0_kernel"}


def group(name):
    return "detector" if name in DET else "tracking" if name in KLT else "pyramid" if name in PYR or "level" in name or "clahe" in name else "other"


def load(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
        if not found:
            sys.exit(f"no *kernel_trace.csv under {path}")
        path = found[-1]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")))
    rows.sort()
    return path, rows


def periods(rows):
    """one entry per keyframe: indices of its stereo kernels; a keyframe's stereo call is the tracking triple that ends
    in epi_gate_kernel"""
    out = []
    last_compact = None
    for i, (_, _, name, _) in enumerate(rows):
        if name == "klt_compact_kernel":
            last_compact = i
        elif name == "epi_gate_kernel" and last_compact is not None:
            out.append((last_compact, i))
    return out


def report(path):
    path, rows = load(path)
    kfs = periods(rows)
    print(f"# {path}: {len(rows)} kernel launches, {len(kfs)} keyframes")
    print("kf  stereo_us  stage2_us  det_start_us  det_end_us  det_us  overlap_us  period_us  | kernel us of the period: "
          "tracking  detector  pyramid  other | queues: tracking / detector / pyramid")
    us = lambda ns: ns / 1000.0
    tot = defaultdict(float)
    n = 0
    for k, (i0, i1) in enumerate(kfs):
        s0, s1 = rows[i0][0], rows[i1][1]
        nxt = rows[kfs[k + 1][0]][0] if k + 1 < len(kfs) else None
        # the chain of this keyframe: detector kernels up to the next keyframe; forked early they start before the stereo
        # kernels end, so look from the stereo start on
        det = [r for r in rows if r[2] in DET and r[0] >= s0 and (nxt is None or r[0] < nxt)]
        stage2 = [r for r in rows[i0:i1 + 1] if r[2] == "klt_stage2_kernel"]
        if not det or nxt is None:
            continue      # the last keyframe has no complete period
        d0, d1 = min(r[0] for r in det), max(r[1] for r in det)
        ov = max(0, min(s1, d1) - max(s0, d0))
        dur, queues = defaultdict(float), defaultdict(set)
        for r in rows:
            if s0 <= r[0] < nxt:
                dur[group(r[2])] += us(r[1] - r[0])
                queues[group(r[2])].add(r[3])
        q = lambda g: ",".join(sorted(queues[g])) or "-"
        st2 = us(stage2[-1][1] - stage2[-1][0]) if stage2 else float("nan")
        print(f"{k:2d}  {us(s1 - s0):9.1f}  {st2:9.1f}  {us(d0 - s0):12.1f}  {us(d1 - s0):10.1f}  {us(d1 - d0):6.1f}  {us(ov):10.1f}  "
              f"{us(nxt - s0):9.1f}  | {dur['tracking']:8.1f}  {dur['detector']:8.1f}  {dur['pyramid']:7.1f}  {dur['other']:5.1f} | "
              f"{q('tracking')} / {q('detector')} / {q('pyramid')}")
        for key, v in (("stereo", us(s1 - s0)), ("stage2", st2), ("det", us(d1 - d0)), ("overlap", us(ov)), ("period", us(nxt - s0)),
                       ("tracking", dur["tracking"]), ("detector", dur["detector"]), ("pyramid", dur["pyramid"]), ("other", dur["other"])):
            tot[key] += v
        n += 1
    if n:
        print("mean " + "  ".join(f"{k} {v / n:.1f}" for k, v in tot.items()) + f"  (us, {n} periods)")
    split(rows, kfs)
    after_keyframe(rows, kfs)


SPLIT = ("klt_compact_kernel", "klt_stage1_kernel", "klt_stage2_kernel", "epi_gate_kernel")


def idle(rows, q, t0, t1):
    """[t0, t1) minus the union of the kernel intervals of queue q (rows are sorted by start)"""
    busy, end = 0, t0
    for r in rows:
        if r[3] == q and r[1] > t0 and r[0] < t1:
            a, b = max(r[0], end), min(r[1], t1)
            if b > a:
                busy += b - a
                end = b
    return t1 - t0 - busy


def quartiles(v):
    """lower quartile, median, upper quartile (linear interpolation between the order statistics)"""
    v = sorted(v)
    def at(p):
        x = p * (len(v) - 1)
        lo = int(x)
        return v[lo] + (v[min(lo + 1, len(v) - 1)] - v[lo]) * (x - lo)
    return at(0.25), at(0.5), at(0.75)


def split(rows, kfs):
    """the stereo interval kernel by kernel (the call's four launches in stream order and the gaps between them) with the
    detector chain's interval beside it, the idle time of the tracking kernels' queue over the period, and the idle time
    of the pyramid builds' queue over the period and inside the stereo interval; then mean and quartiles of every column"""
    us = lambda ns: ns / 1000.0
    cols = ("compact", "gap", "stage1", "gap", "stage2", "gap", "epi_gate")
    print("kf  " + "  ".join(f"{c:>8s}" for c in cols) + "  | stereo_us  det_us  period_us  tracking_queue_idle_us  "
          "pyramid_queue_idle_us  of_it_in_stereo_us")
    names = ("compact", "gap1", "stage1", "gap2", "stage2", "gap3", "epi_gate", "stereo", "det", "period", "tracking_queue_idle",
             "pyramid_queue_idle", "pyramid_queue_idle_in_stereo")
    table = []
    for k, (i0, i1) in enumerate(kfs):
        if k + 1 >= len(kfs):
            continue
        call = [r for r in rows[i0:i1 + 1] if r[2] in SPLIT]
        if [r[2] for r in call] != list(SPLIT):
            continue      # not the plain four-launch call (another call's kernels of the same names in between)
        s0, s1, nxt = call[0][0], call[-1][1], rows[kfs[k + 1][0]][0]
        det = [r for r in rows if r[2] in DET and s0 <= r[0] < nxt]
        if not det:
            continue
        vals = []
        for j, r in enumerate(call):
            vals.append(us(r[1] - r[0]))
            if j + 1 < len(call):
                vals.append(us(call[j + 1][0] - r[1]))
        # the queue the pyramid builds of this period run on (the one that holds most of their kernel time)
        pq = defaultdict(int)
        for r in rows:
            if s0 <= r[0] < nxt and group(r[2]) == "pyramid":
                pq[r[3]] += r[1] - r[0]
        pyr = max(pq, key=pq.get) if pq else None
        vals += [us(s1 - s0), us(max(r[1] for r in det) - min(r[0] for r in det)), us(nxt - s0), us(idle(rows, call[0][3], s0, nxt)),
                 us(idle(rows, pyr, s0, nxt)) if pq else float("nan"), us(idle(rows, pyr, s0, s1)) if pq else float("nan")]
        print(f"{k:2d}  " + "  ".join(f"{v:8.1f}" for v in vals[:len(cols)]) + "  | " + "  ".join(f"{v:9.1f}" for v in vals[len(cols):]))
        table.append(vals)
    if table:
        n = len(table)
        print("mean split " + "  ".join(f"{k} {sum(c) / n:.1f}" for k, c in zip(names, zip(*table))) + f"  (us, {n} periods)")
        print("lower quartile / median / upper quartile  " +
              "  ".join(f"{k} {'/'.join(f'{q:.1f}' for q in quartiles(c))}" for k, c in zip(names, zip(*table))))


def after_keyframe(rows, kfs):
    """what follows a keyframe: the idle time of the tracking queue between the stereo call's epi_gate_kernel and the next
    plain call's klt_compact_kernel, cornerSubPix, the klt_stage1_kernel of that plain call beside the mean of the period's
    other plain calls, and how far subpix_kernel runs past the start of that launch (negative: it ended before)"""
    us = lambda ns: ns / 1000.0
    names = ("idle_before_next_call", "subpix", "next_stage1", "other_stage1_mean", "subpix_past_next_stage1_start")
    print("kf  " + "  ".join(f"{c:>30s}" for c in names))
    table = []
    for k, (i0, i1) in enumerate(kfs):
        if k + 1 >= len(kfs):
            continue
        s0, gate_end, nxt, q = rows[i0][0], rows[i1][1], rows[kfs[k + 1][0]][0], rows[i0][3]
        plain = [r for r in rows if r[3] == q and r[2] in ("klt_compact_kernel", "klt_stage1_kernel") and gate_end <= r[0] < nxt]
        compacts = [r for r in plain if r[2] == "klt_compact_kernel"]
        stage1 = [r for r in plain if r[2] == "klt_stage1_kernel"]
        sub = [r for r in rows if r[2] == "subpix_kernel" and s0 <= r[0] < nxt]
        if not compacts or len(stage1) < 2 or not sub:
            continue
        vals = [us(idle(rows, q, gate_end, compacts[0][0])), us(sub[0][1] - sub[0][0]), us(stage1[0][1] - stage1[0][0]),
                sum(us(r[1] - r[0]) for r in stage1[1:]) / (len(stage1) - 1), us(sub[0][1] - stage1[0][0])]
        print(f"{k:2d}  " + "  ".join(f"{v:30.1f}" for v in vals))
        table.append(vals)
    if table:
        n = len(table)
        print("mean after keyframe " + "  ".join(f"{k} {sum(c) / n:.1f}" for k, c in zip(names, zip(*table))) + f"  (us, {n} periods)")
        print("lower quartile / median / upper quartile  " +
              "  ".join(f"{k} {'/'.join(f'{q:.1f}' for q in quartiles(c))}" for k, c in zip(names, zip(*table))))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for p in sys.argv[1:]:
        report(p)
