"""bench.py with chosen wave priorities: every context bench.py creates gets its level through ov2_ctx_set_wave_prio right
after its creation -- high-priority contexts (the front end by default) --fe-level, the others (the local-BA worker by
default) --ba-level.  A level left out keeps the context's default.  bench.py itself runs unchanged, in this process.
usage: python scripts/wave_prio_bench.py [--fe-level 0..3] [--ba-level 0..3] -- <bench.py arguments>"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)
    own, rest = argv[:cut], argv[cut + 1:]
    levels = {"--fe-level": None, "--ba-level": None}
    for k in range(0, len(own), 2):
        if own[k] not in levels or k + 1 >= len(own):
            sys.exit(__doc__)
        levels[own[k]] = int(own[k + 1])
    from ov2slam_amd import frontend as fe
    create = fe.Context.__init__

    def create_with_level(self, device=0, high_priority=False):
        create(self, device, high_priority)
        level = levels["--fe-level"] if high_priority else levels["--ba-level"]
        if level is not None:
            self.set_wave_prio(level)
        print(f"[wave_prio_bench] {'high' if high_priority else 'normal'}-priority context at wave priority {self.get_wave_prio()}",
              file=sys.stderr, flush=True)

    fe.Context.__init__ = create_with_level
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
