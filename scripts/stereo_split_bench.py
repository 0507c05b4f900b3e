"""bench.py with a chosen split of stereoMatching's no-prior descent: every context bench.py creates gets --split through
ov2_klt_set_stereo_split right after its creation (k >= the pyramid's levels: no split; left out: the library's default).
bench.py itself runs unchanged, in this process.
usage: python scripts/stereo_split_bench.py [--split k] -- <bench.py arguments>"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)
    own, rest = argv[:cut], argv[cut + 1:]
    split = None
    if own:
        if len(own) != 2 or own[0] != "--split":
            sys.exit(__doc__)
        split = int(own[1])
    from ov2slam_amd import frontend as fe
    create = fe.Context.__init__

    def create_with_split(self, device=0, high_priority=False):
        create(self, device, high_priority)
        if split is not None:
            self.set_stereo_split(split)
        print(f"[stereo_split_bench] {'high' if high_priority else 'normal'}-priority context: stereo split "
              f"{'default' if split is None else split}", file=sys.stderr, flush=True)

    fe.Context.__init__ = create_with_split
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
