"""The matrix behind the default CU share of the local-BA worker ("A CU share for the worker").
Runs bench.py unchanged under OV2_WORKER_CUS / OV2_WORKER_CU_LAYOUT, one process per run, each under its own `timeout`;
the first run that fails (or is killed) ends the job.  Settings are visited in order, in reversed order in every second
round.  With --parent DIR (a checkout of the parent commit with its libraries built) the parent's own bench.py and
build run as one more setting, alternating with the others in the same job.

usage: python scripts/cu_share_bench.py [--parent DIR] [--rounds 3] [--steps 20] [--warmup 5] [--limit 240]
                                        [--settings off,255,128s,64s,32s,16s,128p,...] [--no-ba-too] [--out FILE]
  a setting: `off` (OV2_WORKER_CUS=0, the parent's behaviour), or a count followed by s (spread, the default) or p (packed)
  --no-ba-too  also runs `--no-ba` for `parent` and `off` (no masked context exists there)
Prints one line per run and, at the end, per setting: every headline figure, median, min, max, solves/s, and the keep
rule against `parent` (or `off` without --parent): every run above every run of the reference, gain of the medians at
least three times the reference's min-max spread, solves/s at least half the reference's median."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_setting(s):
    if s in ("off", "parent"):
        return s, {"OV2_WORKER_CUS": "0"} if s == "off" else {}
    lay = 1 if s.endswith("p") else 0
    n = int(s.rstrip("sp"))
    return f"{n}{'p' if lay else 's'}", {"OV2_WORKER_CUS": str(n), "OV2_WORKER_CU_LAYOUT": str(lay)}


def run(tree, env_add, extra, a):
    env = dict(os.environ)
    env.pop("OV2_WORKER_CUS", None)
    env.pop("OV2_WORKER_CU_LAYOUT", None)
    env.update(env_add)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.steps),
           "--warmup", str(a.warmup)] + extra
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        print(f"[cu_share_bench] FAILED (exit {r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
        sys.exit(1)      # nothing more is started on the GPU
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    lb = j.get("local_ba") or {}
    return dict(fps=j["value"], solves_per_sec=lb.get("solves_per_sec"), solve_ms=(lb.get("ms_per_batch") or {}).get("solve"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one bench.py run may take")
    ap.add_argument("--settings", default="off,255s,128s,128p,64s,64p,32s,32p,16s,16p")
    ap.add_argument("--no-ba-too", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    settings = [parse_setting(s) for s in a.settings.split(",") if s]
    if a.parent:
        settings.insert(0, parse_setting("parent"))
    res = {name: [] for name, _ in settings}
    noba = {"parent": [], "off": []}
    log = open(a.out, "a") if a.out else None

    def note(rec):
        print("[cu_share_bench] " + json.dumps(rec), flush=True)
        if log:
            log.write(json.dumps(rec) + "\n")
            log.flush()

    for rnd in range(a.rounds):
        order = settings if rnd % 2 == 0 else settings[::-1]
        for name, env in order:
            tree = os.path.abspath(a.parent) if name == "parent" else ROOT
            r = run(tree, env, [], a)
            res[name].append(r)
            note(dict(round=rnd, setting=name, steps=a.steps, **r))
            if a.no_ba_too and name in noba:
                r = run(tree, env, ["--no-ba"], a)
                noba[name].append(r["fps"])
                note(dict(round=rnd, setting=name + " --no-ba", steps=a.steps, fps=r["fps"]))

    ref = "parent" if a.parent else "off"
    rf = [r["fps"] for r in res[ref]]
    rs = [r["solves_per_sec"] for r in res[ref] if r["solves_per_sec"] is not None]
    spread = max(rf) - min(rf)
    print(f"\n{'setting':>8} {'headline frames/s (each run)':<40} {'median':>9} {'min':>9} {'max':>9} {'solves/s':>9} {'solve ms':>9}  keep rule vs {ref}")
    for name, _ in settings:
        f = [r["fps"] for r in res[name]]
        s = [r["solves_per_sec"] for r in res[name] if r["solves_per_sec"] is not None]
        ms = [r["solve_ms"] for r in res[name] if r["solve_ms"] is not None]
        verdict = ""
        if name != ref:
            above = min(f) > max(rf)
            gain = statistics.median(f) - statistics.median(rf)
            enough = gain >= 3.0 * spread
            half = bool(s) and bool(rs) and statistics.median(s) >= 0.5 * statistics.median(rs)
            verdict = (f"all above: {'yes' if above else 'no'}; gain {gain:+.0f} vs 3 x spread {3 * spread:.0f}: {'yes' if enough else 'no'}; "
                       f"solves/s >= half: {'yes' if half else 'no'} -> {'PASS' if above and enough and half else 'fail'}")
        print(f"{name:>8} {' '.join(f'{v:.0f}' for v in f):<40} {statistics.median(f):9.0f} {min(f):9.0f} {max(f):9.0f} "
              f"{statistics.median(s) if s else float('nan'):9.0f} {statistics.median(ms) if ms else float('nan'):9.1f}  {verdict}")
    for name, v in noba.items():
        if v:
            print(f"{name + ' --no-ba':>16} {' '.join(f'{x:.0f}' for x in v)}  median {statistics.median(v):.0f} min {min(v):.0f} max {max(v):.0f}")


if __name__ == "__main__":
    main()
