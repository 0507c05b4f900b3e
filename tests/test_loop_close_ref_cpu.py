"""the checker of the loop-closing tests (tests/loop_close_ref.py) on a hand-made three-keyframe map whose result is written
down with 4 x 4 matrices, and its decision function on the four branches of src/loop_closer.cpp:302-372.  No GPU."""
import numpy as np

import loop_close_ref as R


def _rotz(deg, t):
    a = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    M[:3, 3] = t
    return M


def test_pose_conversions_round_trip():
    for deg, t in ((0, (0, 0, 0)), (35, (1, 2, 3)), (170, (-1, 0, 2)), (-90, (0, 5, 0))):
        M = _rotz(deg, t)
        assert np.abs(R.mat(R.pose7(M)) - M).max() < 1e-15
    assert R.same_pose([1, 2, 3, 0, 0, 0, 1], [1, 2, 3, 0, 0, 0, -1], 0.0)
    assert not R.same_pose([1, 2, 3, 0, 0, 0, 1], [1, 2, 3.001, 0, 0, 0, 1], 1e-6)


def test_update_stage_on_three_keyframes():
    """keyframe 0 constant, 1 the new keyframe (listed), 2 younger.  Landmark 10 is anchored at 1, 11 at 2, 12 at 0, 13 at 1
    with a 2D keypoint, 14 is dead (observed, but not in the map)"""
    T0, T1, T2 = _rotz(0, (0, 0, 0)), _rotz(0, (1, 0, 0)), _rotz(0, (2, 0, 0))
    m = dict(poses={0: R.pose7(T0), 1: R.pose7(T1), 2: R.pose7(T2)},
             points={10: np.array([1.0, 0.0, 4.0]), 11: np.array([2.0, 1.0, 5.0]), 12: np.array([0.0, 0.0, 3.0]),
                     13: np.array([1.5, 0.5, 2.0])},
             obs=[(1, 10), (2, 10), (2, 11), (0, 12), (1, 12), (2, 12), (1, 13), (2, 13), (1, 14), (2, 14)],
             kp3d={10, 11, 12, 14})
    N1 = _rotz(90, (1, 1, 0))                    # the optimised pose of keyframe 1
    poses, points, mc, my, Tc = R.update(m, 1, {1: R.pose7(N1)})
    # written out: keyframe 1 -> N1; keyframe 2 sat at +1 m along x of keyframe 1 and keeps doing so
    assert np.abs(poses[0] - T0).max() == 0 and np.abs(poses[1] - N1).max() < 1e-15
    rel = np.eye(4)
    rel[0, 3] = 1.0
    assert np.abs(poses[2] - N1 @ rel).max() < 1e-15
    assert np.allclose(poses[2][:3, 3], [1, 2, 0], atol=1e-15)        # x of keyframe 1 now points along world y
    # landmark 10: (0, 0, 4) in camera 1 -> N1 * that
    assert np.allclose(points[10], (N1 @ [0, 0, 4, 1])[:3], atol=1e-15) and np.allclose(points[10], [1, 1, 4], atol=1e-15)
    # landmark 11: (0, 1, 5) in camera 2 -> rotated by 90 degrees about z: (-1, 0, 5) + (1, 2, 0)
    assert np.allclose(points[11], [0, 2, 5], atol=1e-15)
    for l in (12, 13):                           # anchored at the constant keyframe / 2D keypoint: untouched, bitwise
        assert np.array_equal(points[l], m["points"][l])
    assert 14 not in points
    assert mc == {10} and my == {11}
    assert np.abs(Tc - N1 @ np.linalg.inv(T1)).max() < 1e-15
    assert R.anchors(m) == {10: 1, 11: 2, 12: 0, 13: 1}


def test_decisions_on_the_four_branches():
    I = [0, 0, 0, 0, 0, 0, 1.0]
    big = R.pose7(_rotz(2.0, (0.3, 0, 0)))
    small = R.pose7(_rotz(0.5, (0.01, 0, 0)))
    pairs = [(5, 5), (7, 9), (3, 3), (8, 2)]
    few = R.decide(29, [10, 12], 30, I, big, pairs, True)
    assert few["branch"] == R.LCL_FEW_PAIRS and few["merged"] == [] and few["loose_start"] is None
    ref = R.decide(30, [12, 10], 30, I, big, pairs, False)
    assert ref["branch"] == R.LCL_PG_REFUSED and ref["inikfid"] == 10 and ref["merged"] == []
    err = np.linalg.norm([0.3, 0, 0, 0, 0, np.deg2rad(2.0)])          # V^-1 t is t to second order in the angle
    assert abs(ref["lc_pose_err"] - err) < 1e-3 and ref["lc_pose_err"] >= 0.02
    clo = R.decide(30, [10, 12], 30, I, small, pairs, True)
    assert clo["branch"] == R.LCL_CLOSED and clo["merged"] == [9, 2] and clo["loose_start"] is None
    assert clo["lc_pose_err"] < 0.02
    loo = R.decide(45, [10, 12], 30, I, big, pairs, True, covis_of_inikf=[4, 8])
    assert loo["branch"] == R.LCL_CLOSED_LOOSE_BA and loo["loose_start"] == 4 and loo["merged"] == [9, 2]
    # an empty covisibility map: the keyframe's own id
    assert R.decide(30, [], 30, I, big, pairs, True, covis_of_inikf=[])["inikfid"] == 30
    assert R.decide(30, [], 30, I, big, pairs, True, covis_of_inikf=[])["loose_start"] == 30
    # |log| of a pure rotation is its angle, of a pure translation its length
    assert abs(R.se3_log_norm(_rotz(40, (0, 0, 0))) - np.deg2rad(40)) < 1e-12
    assert abs(R.se3_log_norm(_rotz(0, (0.3, 0.4, 0))) - 0.5) < 1e-15
