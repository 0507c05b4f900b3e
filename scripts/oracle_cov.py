#!/usr/bin/env python3
"""Line coverage of the CPU oracle under the inputs of a test-helper module (CPU only, gcov).

    python scripts/oracle_cov.py pg_cases                      # tests/pg_cases.py: cases(), run(case, oracle)
    python scripts/oracle_cov.py pg_cases:legacy_cases         # another builder of the same module
    python scripts/oracle_cov.py pg_cases pnp_cases            # several modules, counters added up

A helper module exposes a builder (default `cases`) that returns the cases and `run(case, oracle)` that feeds one case
to the oracle binding.  The oracle and the HIP kernels restate the same algorithms branch for branch, so an oracle line
that never runs under the inputs of the GPU tests marks a kernel branch that no GPU test runs.  The script builds
`make -C oracle cov`, runs the cases in a child process (the counters are written when it exits), and prints the
lines of each oracle source that never ran.  --fail-on FILE exits 1 if FILE has such a line."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = os.path.join(ROOT, "oracle", "_cov")


def child(specs):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import importlib
    from oracle import oracle_py
    oracle_py.lib(os.path.join(COV, "libov2oracle.so"))      # every later call of the binding goes to the coverage build
    for spec in specs:
        name, _, builder = spec.partition(":")
        mod = importlib.import_module(name)
        n = 0
        for case in getattr(mod, builder or "cases")():
            mod.run(case, oracle_py)
            n += 1
        print("%s: %d cases" % (spec, n), file=sys.stderr)


def report(files):
    """{source: (executable lines, [(line number, text) never run])} from gcov's annotated listing"""
    out = {}
    for src in sorted(f for f in os.listdir(os.path.join(ROOT, "oracle")) if f.endswith(".c")):
        if files and src not in files:
            continue
        if not os.path.exists(os.path.join(COV, src[:-2] + ".gcda")):
            continue
        txt = subprocess.run(["gcov", "-t", "-o", COV, src], cwd=os.path.join(ROOT, "oracle"), check=True,
                             capture_output=True, text=True).stdout
        total, missed = 0, []
        for line in txt.splitlines():
            m = re.match(r"\s*([^:]+):\s*(\d+):(.*)", line)
            if not m or m.group(2) == "0":
                continue
            count = m.group(1).strip()
            if count == "-":
                continue
            total += 1
            if count.startswith("#####") or count.startswith("====="):
                missed.append((int(m.group(2)), m.group(3).rstrip()))
        out[src] = (total, missed)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("modules", nargs="+", help="helper module under tests/, optionally module:builder")
    ap.add_argument("--files", nargs="*", default=[], help="oracle sources to report (default: all that ran)")
    ap.add_argument("--fail-on", default=None, help="exit 1 if this oracle source has a line that never ran")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.modules)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "cov"])
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child"] + a.modules)
    rep = report(a.files)
    for src, (total, missed) in rep.items():
        print("%-22s %5.1f %% of %d lines, %d never run" % (src, 100.0 * (total - len(missed)) / max(total, 1), total, len(missed)))
        for no, text in missed:
            print("    %5d: %s" % (no, text.strip()))
    if a.fail_on:
        if a.fail_on not in rep:
            sys.exit("%s: not run at all" % a.fail_on)
        sys.exit(1 if rep[a.fail_on][1] else 0)


if __name__ == "__main__":
    main()
