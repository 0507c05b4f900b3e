"""ov2h_assemble_local_pose_graph (Optimizer::assembleLocalPoseGraph of the C++ host mirror, no GPU context) against the numpy
checker tests/local_pg_ref.py on a synth_filter.make_map(21, 60) map with keyframes removed through ov2h_map_remove_keyframe.

Bar: ids, constness flags and edge indices exact; the listed poses are the stored 7-vectors bit for bit; T_ij agrees with the
4 x 4 product to 1e-12 (scene scale <= 20 m, as in test_map_pg_update_gpu.py)."""
import numpy as np
import pytest

import local_pg_ref as R
from loop_close_ref import mat
from ov2slam_amd import host_map, synth_filter

NK, NL = 21, 60
NEWKF = NK - 4

# (name, removed keyframes, newkf, kfloop_id, expected ids or None)
CASES = [
    ("live_loop", (), NEWKF, 5, list(range(5, NEWKF + 1))),
    ("dead_loop_walks_up", (5, 6), NEWKF, 5, list(range(7, NEWKF + 1))),
    ("dead_inside_range", (8, 9, 12), NEWKF, 5, [k for k in range(5, NEWKF + 1) if k not in (8, 9, 12)]),
    ("dead_newkf", (NEWKF,), NEWKF, 5, None),
    ("loop_is_newkf_minus_1", (), NEWKF, NEWKF - 1, [NEWKF - 1, NEWKF]),
    ("walk_runs_past_newkf", (NEWKF - 2, NEWKF - 1), NEWKF, NEWKF - 2, None),
]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def the_map():
    return synth_filter.make_map(NK, NL)


def new_pose(m, newkf):
    """the stored pose of newkf moved by a small rigid motion (what a loop pose looks like)"""
    p = np.array(m["poses"][newkf], np.float64)
    p[:3] += [0.03, -0.02, 0.025]
    q = np.array([0.01, -0.015, 0.02, 1.0])
    p[3:] = q / np.linalg.norm(q)
    return p


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hook_equals_checker(the_map, case):
    _, dead, newkf, loop, want_ids = case
    m = the_map
    hm = host_map.FilterMap(m)
    for k in dead:
        hm.remove_keyframe(k)
    Tn = new_pose(m, newkf)
    alive = [k for k in range(NK) if k not in dead]
    ref = R.assemble({k: m["poses"][k] for k in alive}, alive, newkf, loop, Tn)
    got = hm.assemble_local_pose_graph(newkf, loop, Tn)
    assert (ref is None) == (want_ids is None)
    if want_ids is None:
        assert got is None
        return
    assert got is not None and got["kfids"].tolist() == want_ids == ref["kfids"].tolist()
    n = len(want_ids)
    for k in ("pose_const", "edge_i", "edge_j"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["pose"].shape == (n, 7) and np.array_equal(got["pose"].view(np.uint64), ref["pose"].view(np.uint64))
    err = max(np.abs(mat(got["T_ij"][e]) - ref["T_ij"][e]).max() for e in range(n))
    print(f"[local_pg_ref {case[0]}] n_pose {n}, max |T_ij - ref| {err:.3e}")
    assert err <= 1e-12
    if n == 2:       # two edges between the same pair: the odometry edge and the closing edge
        assert got["edge_i"].tolist() == [0, 0] and got["edge_j"].tolist() == [1, 1]
        assert np.abs(mat(got["T_ij"][0]) - mat(got["T_ij"][1])).max() > 1e-3


def test_checker_chain_rules():
    """the checker's own rules on bare id sets"""
    alive = [0, 1, 2, 5, 6, 9]
    assert R.chain(alive, 9, 3) == [5, 6, 9]
    assert R.chain(alive, 9, 6) == [6, 9]
    assert R.chain(alive, 9, 7) is None            # the walk stops at newkf itself: one pose
    assert R.chain(alive, 6, 9) is None            # a loop keyframe past newkf
    assert R.chain(alive, 8, 0) is None            # a dead newkf
    assert R.chain(alive, 9, 12) is None           # nothing at or above the loop id
    assert R.chain(alive, 9, -3) == [0, 1, 2, 5, 6, 9]
