#!/usr/bin/env python3
"""Does the keyframe detector chain really run beside the stereo matching?  Reads a `rocprofv3 --kernel-trace
--output-format csv` trace of `bench.py --no-ba` (a run of its own, no counters) and prints, per keyframe period:
  the stereo-matching interval (klt_compact_kernel .. epi_gate_kernel of the keyframe) and its klt_stage2_kernel,
  the detector-chain interval (first det_* kernel .. subpix_kernel), both relative to the start of the stereo interval,
  their overlap, the length of the period (stereo start to the next stereo start), and the summed kernel durations of
  the period by group (tracking + stereo, detector chain, pyramid builds, everything else) with the hardware queues
  each group ran on -- two groups that share a queue cannot overlap.
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


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for p in sys.argv[1:]:
        report(p)
