#!/usr/bin/env python3
"""Does the tracking stream wait for the pyramid stream?  Reads a `rocprofv3 --kernel-trace --output-format csv` trace of
`bench.py --no-ba --steps 6 --warmup 2 --no-cpu-baseline --no-euroc-like --no-hard-stream` (a run of its own, no
counters; the input of kf_overlap_trace.py) and prints
  per tracking or stereo call (a klt_compact_kernel and the tracking kernels that follow it): its start, the idle time of
  its hardware queue in front of it, the number of wait packets the call put in front of its kernels, the end stamp of
  the last kernel of the pyramid build it consumes, and the difference between that end and the call's start -- a call
  that starts a few us behind its build's end was waiting for it;
  per keyframe period (stereo start to the next stereo start): the idle time of the tracking queue and of the pyramid
  queue, how much of the pyramid queue's idle time lies inside the stereo interval, the number of calls that start
  within 10 us of their build's end, the summed kernel durations by group and the hardware queues of each group.
Builds and calls are paired by count, the order bench.py's Workload.step enqueues them in: every call consumes the next
build (a tracking call the left pyramid of its frame, the stereo call of a keyframe the right one); a stereo call with
no tracking call in front of it (the first frame) skips one build, its own left pyramid.
Wait packets are no kernels and leave no row in a kernel trace: the column follows from the same pairing and the pool's
rule (ov2_pyr_wait_ready: the main stream waits once per build), so a call issues one packet per build it is the first
to consume, the host running ahead of the device as it does in this bench.  ov2_ctx_pyr_wait_stats has the measured
totals.  --every-wait gives the column for a library from before that rule: one packet per pyramid a call reads, two per call.
usage: pyr_wait_trace.py [--every-wait] <kernel_trace.csv or a directory holding one> [more traces ...]"""
import os
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kf_overlap_trace import group as _group, load, short  # noqa: E402,F401  (short: load() names kernels with it)

NEAR_NS = 10_000          # "starts behind its build's end": within 10 us
BUILD_HEAD = {"clahe_lut_wave_kernel", "clahe_lut_kernel"}   # first kernel of a build with CLAHE on


def group(name):
    """kf_overlap_trace.group, with the pyrDown kernels of a build counted as pyramid work"""
    return "pyramid" if name.startswith("pyrdown") else _group(name)


def busy_ns(spans, lo, hi):
    """length of the union of the (start, end) spans clipped to [lo, hi)"""
    total, cur_s, cur_e = 0, None, None
    for s, e in sorted((max(s, lo), min(e, hi)) for s, e in spans if e > lo and s < hi):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                total += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        total += cur_e - cur_s
    return total


def analyse(rows, every_wait=False):
    """rows = load()'s (start ns, end ns, kernel, queue), sorted by start.  Returns (calls, periods, notes): a dict per
    tracking / stereo call and per complete keyframe period, times in ns.  every_wait: the library waits for every
    pyramid a call reads (two packets per call) instead of once per build."""
    notes = []
    # ---- builds: runs of pyramid kernels, a new one at every CLAHE table kernel
    builds = []
    for s, e, name, q in rows:
        if group(name) != "pyramid" or name == "level_kernel":     # level_kernel: gradient planes on demand, not a build
            continue
        if name in BUILD_HEAD or not builds:
            builds.append(dict(start=s, end=e, queue=q))
        else:
            builds[-1]["end"] = max(builds[-1]["end"], e)
    # ---- calls: klt_compact_kernel and the tracking kernels up to the next one
    calls = []
    for i, (s, e, name, q) in enumerate(rows):
        if group(name) != "tracking":
            continue
        if name == "klt_compact_kernel":
            calls.append(dict(first=i, start=s, end=e, queue=q, stereo=False))
        elif calls:
            calls[-1]["end"] = max(calls[-1]["end"], e)
            calls[-1]["stereo"] |= name == "epi_gate_kernel"
    last_end = {}          # queue -> end of the last kernel seen on it
    k, nb, prev_was_tracking = 0, 0, False
    for i, (s, e, name, q) in enumerate(rows):
        if k < len(calls) and calls[k]["first"] == i:
            c = calls[k]
            c["idle_before"] = max(0, s - last_end[q]) if q in last_end else None
            c["waits"] = 1                                           # the build paired with the call: first consumed here
            if c["stereo"] and not prev_was_tracking:
                nb += 1                                              # its own left pyramid, consumed by no call before it
                c["waits"] += 1
            elif k == 0:
                c["waits"] += 1                                      # a trace that opens with a tracking call: prev as well
            if every_wait:
                c["waits"] = 2
            c["build"] = nb if nb < len(builds) else None
            c["build_end"] = builds[nb]["end"] if nb < len(builds) else None
            c["gap"] = s - builds[nb]["end"] if nb < len(builds) else None
            nb += 1
            prev_was_tracking = not c["stereo"]
            k += 1
        last_end[q] = max(last_end.get(q, 0), e)
    if nb != len(builds):
        notes.append(f"{len(builds)} builds in the trace, the calls account for {nb}: the pairing by count may be off")
    early = sum(1 for c in calls if c["gap"] is not None and c["gap"] < 0)
    if early:
        notes.append(f"{early} calls start before the end of the build paired with them: the pairing by count is off")
    # ---- keyframe periods
    st = [c for c in calls if c["stereo"]]
    periods = []
    for a, b in zip(st, st[1:]):
        lo, hi = a["start"], b["start"]
        inside = [r for r in rows if lo <= r[0] < hi]
        queues, dur = defaultdict(set), defaultdict(int)
        for s, e, name, q in inside:
            queues[group(name)].add(q)
            dur[group(name)] += e - s
        tq, pq = queues["tracking"], queues["pyramid"]
        # spans of every kernel on those queues that reaches into the period (a kernel launched before it may still run)
        spans_t = [(s, e) for s, e, _, q in rows if q in tq]
        spans_p = [(s, e) for s, e, _, q in rows if q in pq]
        mine = [c for c in calls if lo <= c["start"] < hi]
        periods.append(dict(start=lo, period=hi - lo, stereo=a["end"] - lo,
                            track_idle=(hi - lo) - busy_ns(spans_t, lo, hi),
                            pyr_idle=(hi - lo) - busy_ns(spans_p, lo, hi),
                            pyr_idle_in_stereo=(a["end"] - lo) - busy_ns(spans_p, lo, a["end"]),
                            calls=len(mine), near=sum(1 for c in mine if c["gap"] is not None and 0 <= c["gap"] <= NEAR_NS),
                            dur=dict(dur), queues={g: sorted(v) for g, v in queues.items()}))
    return calls, periods, notes


def report(path, per_periods=3, every_wait=False):
    path, rows = load(path)
    calls, periods, notes = analyse(rows, every_wait)
    us = lambda ns: float("nan") if ns is None else ns / 1000.0
    t0 = rows[0][0] if rows else 0
    print(f"# {path}: {len(rows)} kernel launches, {len(calls)} tracking / stereo calls, {len(periods)} complete keyframe periods")
    for n in notes:
        print("# note: " + n)
    # the calls of the last complete periods: the steady state, past the warm-up
    shown = periods[-per_periods:]
    lo, hi = (shown[0]["start"], shown[-1]["start"] + shown[-1]["period"]) if shown else (0, 0)
    print("call  kind      start_us  queue  idle_before_us  wait_packets  build  build_end_us  start_minus_build_end_us")
    for n, c in enumerate(calls):
        if not lo <= c["start"] < hi:
            continue
        print(f"{n:4d}  {'stereo  ' if c['stereo'] else 'tracking'}  {us(c['start'] - t0):10.1f}  {c['queue']:>5}  "
              f"{us(c['idle_before']):14.1f}  {c['waits']:12d}  {str(c['build']):>5}  {us(None if c['build_end'] is None else c['build_end'] - t0):12.1f}  "
              f"{us(c['gap']):10.1f}")
    print("kf  period_us  stereo_us  track_idle_us  pyr_idle_us  pyr_idle_in_stereo_us  calls  within_10us | kernel us: "
          "tracking  detector  pyramid  other | queues: tracking / detector / pyramid")
    tot = defaultdict(float)
    for k, p in enumerate(periods):
        d, q = p["dur"], lambda g: ",".join(p["queues"].get(g, [])) or "-"
        print(f"{k:2d}  {us(p['period']):9.1f}  {us(p['stereo']):9.1f}  {us(p['track_idle']):13.1f}  {us(p['pyr_idle']):11.1f}  "
              f"{us(p['pyr_idle_in_stereo']):21.1f}  {p['calls']:5d}  {p['near']:11d} | {us(d.get('tracking', 0)):8.1f}  "
              f"{us(d.get('detector', 0)):8.1f}  {us(d.get('pyramid', 0)):7.1f}  {us(d.get('other', 0)):5.1f} | "
              f"{q('tracking')} / {q('detector')} / {q('pyramid')}")
        for key in ("period", "stereo", "track_idle", "pyr_idle", "pyr_idle_in_stereo"):
            tot[key] += us(p[key])
        for g in ("tracking", "detector", "pyramid", "other"):
            tot[g] += us(d.get(g, 0))
        tot["calls"] += p["calls"]
        tot["within_10us"] += p["near"]
    if periods:
        n = len(periods)
        print("mean " + "  ".join(f"{k} {v / n:.1f}" for k, v in tot.items()) + f"  (us / counts per period, {n} periods)")
        plain = [c for c in calls if not c["stereo"] and c["gap"] is not None and c["start"] >= periods[0]["start"]]
        if plain:
            gaps = sorted(us(c["gap"]) for c in plain)
            print(f"plain tracking calls: {len(plain)}, start minus build end: lower quartile {gaps[len(gaps) // 4]:.1f} us, median "
                  f"{gaps[len(gaps) // 2]:.1f} us, upper quartile {gaps[3 * len(gaps) // 4]:.1f} us, within 10 us: "
                  f"{sum(1 for g in gaps if 0 <= g <= 10.0)}, within 20 us: {sum(1 for g in gaps if 0 <= g <= 20.0)}, idle in front: mean "
                  f"{sum(us(c['idle_before']) for c in plain) / len(plain):.1f} us, wait packets per call: "
                  f"{sum(c['waits'] for c in plain) / len(plain):.2f}")
        st = [c for c in calls if c["stereo"] and c["start"] >= periods[0]["start"] and c["idle_before"] is not None]
        if st:
            print(f"stereo calls: {len(st)}, idle in front: mean {sum(us(c['idle_before']) for c in st) / len(st):.1f} us, wait packets "
                  f"per call: {sum(c['waits'] for c in st) / len(st):.2f}")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--every-wait"]
    if not args:
        sys.exit(__doc__)
    for p in args:
        report(p, every_wait="--every-wait" in sys.argv[1:])
