"""CPU tests of the checker of the structure-only BA on the map mirrors (tests/structure_ba_ref.py) and of its cases
(tests/structure_ba_cases.py): the selection rules on a hand-built table, every case held to the branch of the minimiser it is
there for, and every case shown to be TAME -- a copy whose initial points are moved by 1e-13 takes the same sequence of
step_is_valid / step_is_successful flags, ends at the same cost to 1e-11 relative and at the same points within a tenth of the
tolerance the GPU tests use (1e-9 * max(1, |x|_inf)).  Only then is a comparison of points between two correct
implementations meaningful.  Measured on the oracle: the copies of `w10x400` differ by 5e-11 in the points, of `thin` by
4e-12, of `w10x2600` by 1.5e-11, of `rejected` (noise 2 m, three rejected steps) by 1e-14; with 8 m of noise on the first shape
they differ by 5e-6, which is why the cases stay at 0.02-0.1 m but for the one on the smallest window."""
import functools

import numpy as np
import pytest

from ov2slam_amd import ba_types as T
import structure_ba_cases as SC
import structure_ba_ref as SR

POINT_TOL = 1e-9   # of the GPU tests, times max(1, |x|_inf)


def flags_of(R):
    return [(int(i["valid"]), int(i["ok"])) for i in R.log]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's solve of the case, computed once: dict(points, ids, counts, result (BaResult), flags)"""
    from oracle import oracle_py
    oracle_py.build()
    d, scale = SC.tables_of(name)
    P, R, counts, entered = SR.solve(oracle_py, d, scale, SC.problem_of(name)[2], SC.cam_of(name), SC.CASES[name]["max_iters"])
    return dict(points=P.lm.copy(), ids=np.array(entered, np.int32), counts=counts, result=R, flags=flags_of(R))


def point_error(a, b):
    """max over the points of |a - b|_inf / max(1, |b|_inf)"""
    return float((np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b).max(1))).max()) if len(a) else 0.0


def hand_table():
    """4 keyframes (3 is dead), 6 landmarks: 0 alive 3D with rows out of keyframe order; 1 alive 3D with a dead row, a row in
    the dead keyframe and one live row; 2 dead with a row; 3 alive, not 3D, with a row; 4 alive 3D without rows; 5 alive 3D
    whose only row is dead"""
    rows = [  # kf, lm, flag, scale
        (2, 0, 3, 1), (1, 1, 0, 0), (0, 0, 1, 0), (3, 1, 1, 0), (1, 0, 3, 2), (0, 2, 1, 0), (2, 1, 3, 0), (0, 3, 1, 0), (1, 5, 0, 0)]
    n = len(rows)
    d = dict(kf_pose=np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (4, 1)), kf_state=np.array([1, 1, 1, 0], np.uint8),
             lm_xyz=np.arange(18, dtype=np.float64).reshape(6, 3) + 5.0, lm_state=np.array([3, 3, 0, 1, 3, 3], np.uint8),
             obs_kf=np.array([r[0] for r in rows], np.int32), obs_lm=np.array([r[1] for r in rows], np.int32),
             obs_flag=np.array([r[2] for r in rows], np.uint8), obs_uv=np.arange(2 * n, dtype=np.float64).reshape(n, 2),
             obs_ruv=100.0 + np.arange(2 * n, dtype=np.float64).reshape(n, 2))
    d["kf_pose"][:, 0] = np.arange(4)
    return d, np.array([r[3] for r in rows], np.int32)


def test_selection_rules_on_a_hand_built_table():
    d, scale = hand_table()
    ids = [0, 99, -1, 2, 3, 1, 0, 4, 5]
    cam = (np.array([400.0, 400, 320, 240]), np.array([410.0, 410, 330, 250]), np.array([-0.1, 0, 0, 0, 0, 0, 1.0]))
    P, counts, entered = SR.flat_problem(d, scale, ids, cam)
    assert entered == [0, 1]
    assert counts == dict(n_listed=9, n_lm=2, n_skipped=7, n_res=7)
    # landmark 0: keyframes 0 (mono), 1 (stereo, scale 2), 2 (stereo, scale 1); landmark 1: keyframe 2 (stereo) alone
    assert P.res_pose.tolist() == [0, 1, 1, 2, 2, 2, 2] and P.res_lm.tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert P.res_type.tolist() == [T.L_XYZ, T.L_XYZ, T.R_XYZ, T.L_XYZ, T.R_XYZ, T.L_XYZ, T.R_XYZ]
    assert P.res_sigma.tolist() == [1, 4, 4, 2, 2, 1, 1]
    assert P.res_uv.tolist() == [[4, 5], [8, 9], [108, 109], [0, 1], [100, 101], [12, 13], [112, 113]]
    assert np.array_equal(P.lm, d["lm_xyz"][[0, 1]]) and P.pose_const.all() and not P.inv_depth
    # a list that names nothing that enters
    _, counts, entered = SR.flat_problem(d, scale, [2, 3, 4, 5, 7], cam)
    assert entered == [] and counts == dict(n_listed=5, n_lm=0, n_skipped=5, n_res=0)


def test_row_order_of_the_table_does_not_matter():
    d, scale = hand_table()
    perm = np.array([4, 2, 0, 6, 1, 3, 5, 8, 7])
    d2 = dict(d)
    for k in ("obs_kf", "obs_lm", "obs_flag", "obs_uv", "obs_ruv"):
        d2[k] = d[k][perm]
    cam = (np.ones(4), np.ones(4), np.array([0, 0, 0, 0, 0, 0, 1.0]))
    A, B = SR.flat_problem(d, scale, [1, 0], cam)[0], SR.flat_problem(d2, scale[perm], [1, 0], cam)[0]
    for k in ("res_type", "res_pose", "res_lm", "res_uv", "res_sigma", "lm"):
        assert np.array_equal(getattr(A, k), getattr(B, k)), k


@pytest.mark.parametrize("name", SC.SHAPES + SC.BRANCHES)
def test_case_holds_its_branch(name):
    c, ref = SC.CASES[name], reference(name)
    R, flags = ref["result"], ref["flags"]
    print(name, ref["counts"], T.TERM[R.c.termination], flags, R.c.initial_cost, R.c.final_cost)
    assert ref["counts"]["n_lm"] == len(SC.problem_of(name)[2]) and ref["counts"]["n_skipped"] == 0
    assert flags[0] == (1, 1) and R.c.n_log <= 1 + c["max_iters"]
    if c["term"]:
        assert T.TERM[R.c.termination] == c["term"]
    if T.TERM[R.c.termination] == "function_tolerance":
        assert flags[-1] == (1, 0)
    if name == "w10x400":
        assert R.c.n_log == 5 and ref["counts"]["n_res"] == 3372
    if name == "maxiter3":
        assert R.c.n_log == 4 and reference("w10x400")["result"].c.n_log > 4
    if name in ("iters0", "iters1"):
        assert R.c.n_log == 1 + c["max_iters"]
    if name == "iters0":
        assert R.c.final_cost == R.c.initial_cost and np.array_equal(ref["points"], SC.tables_of(name)[0]["lm_xyz"][ref["ids"]])
    if c["rejected"]:
        assert (1, 0) in flags[:-1] and (1, 1) in flags[flags.index((1, 0)):]
    if name == "w10x2600":
        assert ref["counts"]["n_lm"] == 1300
    if name == "w40x60":
        Q = SR.flat_problem(*SC.tables_of(name), SC.problem_of(name)[2], SC.cam_of(name))[0]
        rows = np.bincount(Q.res_lm[Q.res_type == T.L_XYZ])
        assert rows.max() == 40 and (rows <= 16).any()   # three 16-lane chunks of rows, and points that fill less than one
    if name == "thin":
        per = np.bincount(SR.flat_problem(*SC.tables_of(name), SC.problem_of(name)[2], SC.cam_of(name))[0].res_lm)
        assert (per[:10] == 1).all() and (per[10:20] == 2).all()
    if name == "mono":
        assert not (SC.tables_of(name)[0]["obs_flag"] & 2).any()


@pytest.mark.parametrize("name", SC.SHAPES + SC.BRANCHES)
def test_case_is_tame(oracle, name):
    ref = reference(name)
    d, scale = SC.tables_of(name)
    ids = SC.problem_of(name)[2]
    d = {k: v.copy() for k, v in d.items()}
    d["lm_xyz"][ids] += np.random.default_rng(1).uniform(-1e-13, 1e-13, (len(ids), 3))
    P, R, _, _ = SR.solve(oracle, d, scale, ids, SC.cam_of(name), SC.CASES[name]["max_iters"])
    err = point_error(P.lm, ref["points"])
    print(name, "points", err, "cost", abs(R.c.final_cost / ref["result"].c.final_cost - 1))
    assert flags_of(R) == ref["flags"] and R.c.termination == ref["result"].c.termination
    assert R.c.final_cost == pytest.approx(ref["result"].c.final_cost, rel=1e-11)
    assert err <= 0.1 * POINT_TOL
