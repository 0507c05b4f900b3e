#!/usr/bin/env python3
"""Bitwise A/B of two builds of libov2hip.so on the same seeded calls -- GPU box.  For a change that must not move a
result (a refactor of device code whose assembly came out different): every case runs once under each library
(OV2SLAM_HIP_LIB selects it), in a process of its own with its own time limit, writes its outputs as .npy files, and
the two directories are compared with np.array_equal on the integer views.  The first non-zero exit ends the run.

    lib_parity.py run LIB_A LIB_B OUTDIR [case ...]     both libraries, then the comparison
    lib_parity.py dump OUTDIR case                      one case under the library the environment selects
    lib_parity.py compare DIR_A DIR_B

Sizes are those of smoke(): the smallest that reach every branch."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/ is on the path for two builders of test inputs that the issue names as cases: chain() of tests/test_oracle_pg.py
# (case_pg) and _scene() of tests/test_match.py (case_match); both are imported inside their case
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

ITER = ("cost", "cost_change", "radius", "relative_decrease", "model_cost_change", "step_is_valid", "step_is_successful")


def iter_log(c):
    """the iteration log of a BaResultC / PgResultC as an (n_log, 7) array"""
    return np.array([[float(getattr(i, f)) for f in ITER] for i in c.log[:c.n_log]], np.float64).reshape(-1, len(ITER))


def case_pnp(ctx):
    from ov2slam_amd import synth_ba
    from ov2slam_amd.multi_view_geometry import MultiViewGeometry
    q = synth_ba.make_pnp(200, seed=2)
    ok, T, idx = MultiViewGeometry(ctx).ceresPnP(q["unpx"], q["wpts"], q["Twc0"], 5, 5.9915, True, True, *q["K"])
    return dict(ok=np.array([ok]), T=T, idx=idx)


def case_ba(ctx):
    from ov2slam_amd import local_ba, synth_ba
    out = {}
    for name, inv in (("inv", True), ("xyz", False)):
        P = synth_ba.make_window(8, 300, inv_depth=inv, seed=1)
        R = local_ba.Optimizer(ctx).localBA(P)
        out.update({f"{name}_pose": P.pose, f"{name}_lm": P.lm, f"{name}_chi2": R.chi2, f"{name}_outlier": R.outlier,
                    f"{name}_depth": R.depth_positive, f"{name}_log": iter_log(R.c),
                    f"{name}_cost": np.array([R.c.initial_cost, R.c.final_cost, R.c.l2_initial_cost, R.c.l2_final_cost])})
    return out


def case_pg(ctx):
    from ov2slam_amd import pose_graph
    from test_oracle_pg import chain
    # drift 0.01 rad per keyframe: every Plus takes the branch above the small-angle threshold (theta^2 >= 1e-20)
    P, _ = chain(np.random.default_rng(8), 8, drift=0.01)
    R = pose_graph.solve(ctx, P)
    return dict(pose=P.pose, log=iter_log(R), cost=np.array([R.initial_cost, R.final_cost]), term=np.array([R.termination]))


def case_map(ctx):
    """set-up -> solve -> update on one map, temporal triangulation on a copy whose newest landmarks went back to 2D,
    the keyframe filter last; the tables after each stage"""
    import ctypes as C
    from ov2slam_amd import device_map as DM, local_ba, synth_ba
    W = synth_ba.make_window(12, 600, inv_depth=True, seed=3, max_obs=6)
    out = {}

    def tables(tag, dm):
        out.update({f"{tag}_{k}": v for k, v in dm.download().items()})
    dm = DM.DeviceMap.from_problem(ctx, W, isobs="newest")
    views = DM.setup_batch(ctx, [dm], calib_l=synth_ba.K_L)
    out.update({f"setup_{k}": np.asarray(v) for k, v in DM.fetch_view(ctx, views[0], True).items()})
    pcs, rcs = DM.problems_of(views, W, True)
    o = local_ba.default_options()
    assert ctx.lib.ov2_ba_solve_batch_dev(ctx.h, 1, pcs, C.byref(o), rcs) == 0
    out.update({f"solved_{k}": np.asarray(v) for k, v in DM.fetch_view(ctx, views[0], True).items()})
    upd = DM.update_batch(ctx, [dm], views, cur_kfid=[dm.newkf])[0]
    out.update(update_removed_lmid=upd["removed_lmid"], update_removed_obs=upd["removed_obs"][np.lexsort(upd["removed_obs"].T[::-1])],
               update_stereo_off=upd["stereo_off"][np.lexsort(upd["stereo_off"].T[::-1])])
    tables("updated", dm)
    dm.close()

    dm = DM.DeviceMap.from_problem(ctx, W, isobs="newest")
    t0 = dm.download()
    two_d = np.unique(t0["obs_lm"][t0["obs_kf"] == dm.newkf])[::2].astype(np.int32)   # half of the newest keyframe's landmarks
    dm.set_landmarks(two_d, np.zeros((len(two_d), 3)), np.full(len(two_d), DM.LM_ALIVE | DM.LM_OBS, np.uint8))
    t = dm.triangulate_temporal_batch(calib_l=synth_ba.K_L, stereo=True, max_reproj_err=3.0)[0]
    assert len(t["good_lmid"]) > 0, "the temporal stage triangulated nothing"
    out.update({f"temporal_{k}": np.asarray(v) for k, v in t.items()})
    tables("temporal", dm)
    f = dm.filter_keyframes_batch()[0]
    out.update({f"filter_{k}": np.asarray(v) for k, v in f.items()})
    tables("filtered", dm)
    dm.close()
    return out


def case_match(ctx):
    from ov2slam_amd import mapper
    from test_match import _scene
    inp = _scene(1, n_kp=300, n_cand=1500)[0]
    mc, md = mapper.matchToMap(ctx, inp, 2.0, 0.2)
    return dict(cand=mc, dist=md)


def case_tri(ctx):
    from ov2slam_amd import synth_tri
    from ov2slam_amd.multi_view_geometry import MultiViewGeometry
    out = {}
    for method in (0, 1):
        s = synth_tri.make_pairs(1, seed=2, G=1, rectified=(method == 1), outlier_frac=0.15)
        g = MultiViewGeometry(ctx).triangulate_pairs(s["T_ab"], s["bv_a"], s["bv_b"], s["unpx_a"], s["unpx_b"], s["K_a"], s["K_b"], 3.0,
                                                     method=method, Twc_a=s["Twc_a"], grp=s["grp"], want_parallax=True)
        out.update({f"m{method}_{k}": g[k] for k in ("status", "pt_a", "wpt", "parallax")})
    return out


def case_front(ctx):
    """cornerSubPix and forward-backward KLT at 3 / 8 / 16 lanes per keypoint, 256 keypoints"""
    from ov2slam_amd import frontend as fe, synth
    S = synth.StereoStream()
    p0, p1 = fe.preprocess_image(ctx, S.left(0)), fe.preprocess_image(ctx, S.left(6))
    kps = synth.grid_keypoints(256)
    out = {}
    for lanes in (3, 8, 16):
        ctx.set_klt_lanes(lanes)
        xy, st = fe.FeatureTracker(ctx, 30, 0.01).fbKltTracking(p0, p1, 9, 3, 30.0, 0.5, kps, kps)
        out.update({f"klt{lanes}_xy": xy, f"klt{lanes}_status": st})
    ctx.set_klt_lanes(0)
    out["detect"] = fe.FeatureExtractor(ctx, nmaxdist=35, dmaxquality=0.001).detectSingleScale(p1, xy[st])   # ends in cornerSubPix
    return out


CASES = dict(pnp=(case_pnp, 120), ba=(case_ba, 180), pg=(case_pg, 120), map=(case_map, 180), match=(case_match, 180),
             tri=(case_tri, 120), front=(case_front, 180))   # (function, time limit in seconds)


def dump(outdir, name):
    from ov2slam_amd import frontend as fe
    ctx = fe.Context(0)
    d = os.path.join(outdir, name)
    os.makedirs(d, exist_ok=True)
    for k, v in CASES[name][0](ctx).items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(v))


def compare(a, b):
    def arrays(d):
        return {os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs}
    bad = n = 0
    for rel in sorted(arrays(a) | arrays(b)):   # an array that only one library wrote counts as a difference
        pa, pb = os.path.join(a, rel), os.path.join(b, rel)
        n += 1
        if not (os.path.exists(pa) and os.path.exists(pb)):
            bad += 1
            print(f"DIFFER {rel} only under {a if os.path.exists(pa) else b}", flush=True)
            continue
        x, y = np.load(pa), np.load(pb)
        same = x.shape == y.shape and x.dtype == y.dtype and \
            np.array_equal(x.view(np.uint8).reshape(-1), y.view(np.uint8).reshape(-1))
        bad += not same
        print(f"{'equal ' if same else 'DIFFER'} {rel} {x.dtype}{list(x.shape)}", flush=True)
    print(f"{n - bad} / {n} arrays bitwise equal", flush=True)
    return 1 if bad or not n else 0


def run(lib_a, lib_b, outdir, names):
    for name in names:
        for tag, lib in (("a", lib_a), ("b", lib_b)):
            env = dict(os.environ, OV2SLAM_HIP_LIB=os.path.abspath(lib))
            cmd = [sys.executable, os.path.abspath(__file__), "dump", os.path.join(outdir, tag), name]
            print(f"[{name}] {lib}", flush=True)
            try:
                rc = subprocess.run(cmd, env=env, timeout=CASES[name][1]).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"[{name}] {lib}: exit {rc} -- stopping", flush=True)
                return rc
    return compare(os.path.join(outdir, "a"), os.path.join(outdir, "b"))


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 4 and a[0] == "run":
        sys.exit(run(a[1], a[2], a[3], a[4:] or list(CASES)))
    if len(a) == 3 and a[0] == "dump":
        sys.exit(dump(a[1], a[2]))
    if len(a) == 3 and a[0] == "compare":
        sys.exit(compare(a[1], a[2]))
    sys.exit(__doc__)
