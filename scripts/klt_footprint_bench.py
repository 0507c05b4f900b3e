"""A/B of library builds under the headline benchmark ("Tracking kernels: a footprint that leaves room
beside the solver").  Runs bench.py unchanged with OV2SLAM_HIP_LIB pointing at each build in turn, one process per run, each
under its own `timeout`; the first run that fails (or is killed) ends the job.  Builds are visited in order, in reversed
order in every second round; every build runs the headline, then (--no-ba-too) `--no-ba`, then (--unmasked-too) the headline
with OV2_WORKER_CUS=0.

usage: python scripts/klt_footprint_bench.py name=path/to/lib.so [name=... ...] [--rounds 3] [--steps 20] [--warmup 5]
                                             [--limit 240] [--no-ba-too] [--unmasked-too] [--no-headline] [--full] [--out FILE]
  the first build is the reference (the parent commit's library); `name=` alone is the in-tree library
  --full  passes --full --no-cpu-baseline --no-euroc-like to bench.py and reports its hard_stream figure beside the headline
Prints one line per run and, at the end, per build and mode: every figure, median, min, max and the keep rule against the
reference: every headline run above every headline run of the reference, the --no-ba median not below the reference's
min-max range; the gain of the medians as a multiple of the reference's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(lib, env_add, extra, a):
    env = dict(os.environ)
    for k in ("OV2_WORKER_CUS", "OV2_WORKER_CU_LAYOUT", "OV2SLAM_HIP_LIB"):
        env.pop(k, None)
    if lib:
        env["OV2SLAM_HIP_LIB"] = os.path.abspath(lib)
    env.update(env_add)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps),
           "--warmup", str(a.warmup)] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        print(f"[klt_footprint_bench] FAILED (exit {r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
        sys.exit(1)      # nothing more is started on the GPU
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    lb = j.get("local_ba") or {}
    out = dict(fps=j["value"], solves_per_sec=lb.get("solves_per_sec"), solve_ms=(lb.get("ms_per_batch") or {}).get("solve"))

    def find(o, key):     # --full: the hard-stream figure, wherever the result line keeps it
        if isinstance(o, dict):
            for k, v in o.items():
                if k == key:
                    return v
                f = find(v, key)
                if f is not None:
                    return f
        return None
    hs = find(j, "hard_stream")
    if hs is not None:
        out["hard_stream"] = hs.get("frames_per_sec_front_end_alone") if isinstance(hs, dict) else hs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs="+")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one bench.py run may take")
    ap.add_argument("--no-ba-too", action="store_true")
    ap.add_argument("--unmasked-too", action="store_true")
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    builds = [b.split("=", 1) for b in a.builds]
    modes = ([] if a.no_headline else [("headline", {}, [])]) + ([("--no-ba", {}, ["--no-ba"])] if a.no_ba_too else []) + \
            ([("unmasked", {"OV2_WORKER_CUS": "0"}, [])] if a.unmasked_too else [])
    extra_all = ["--full", "--no-cpu-baseline", "--no-euroc-like"] if a.full else []
    res = {(n, m): [] for n, _ in builds for m, _, _ in modes}
    log = open(a.out, "a") if a.out else None
    for rnd in range(a.rounds):
        for name, lib in (builds if rnd % 2 == 0 else builds[::-1]):
            for mode, env, extra in modes:
                r = run(lib, env, extra + extra_all, a)
                res[(name, mode)].append(r)
                rec = dict(round=rnd, build=name, mode=mode, steps=a.steps, **r)
                print("[klt_footprint_bench] " + json.dumps(rec), flush=True)
                if log:
                    log.write(json.dumps(rec) + "\n")
                    log.flush()
    ref = builds[0][0]
    for mode, _, _ in modes:
        rf = [r["fps"] for r in res[(ref, mode)]]
        spread = max(rf) - min(rf)
        print(f"\n{mode}: {'build':>8} {'frames/s (each run)':<40} {'median':>9} {'min':>9} {'max':>9} {'solves/s':>9}  against {ref}")
        for name, _ in builds:
            f = [r["fps"] for r in res[(name, mode)]]
            s = [r["solves_per_sec"] for r in res[(name, mode)] if r["solves_per_sec"] is not None]
            verdict = ""
            if name != ref:
                gain = statistics.median(f) - statistics.median(rf)
                mult = f"{gain / spread:.1f} x spread {spread:.0f}" if spread > 0 else "spread 0"
                if mode == "--no-ba":
                    verdict = f"gain {gain:+.0f} ({mult}); median not below the reference's range: {'yes' if statistics.median(f) >= min(rf) else 'NO'}"
                else:
                    verdict = f"gain {gain:+.0f} ({mult}); all above: {'yes' if min(f) > max(rf) else 'no'}"
            print(f"{name:>15} {' '.join(f'{v:.0f}' for v in f):<40} {statistics.median(f):9.0f} {min(f):9.0f} {max(f):9.0f} "
                  f"{statistics.median(s) if s else float('nan'):9.0f}  {verdict}")
            hs = [r["hard_stream"] for r in res[(name, mode)] if "hard_stream" in r]
            if hs:
                print(f"{'':>15} hard_stream: {hs}")


if __name__ == "__main__":
    main()
