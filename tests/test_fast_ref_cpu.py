"""The checker of the whole-image FAST detector (tests/fast_ref.py) held to independent formulas, without a GPU: the score
against the plain segment test swept over the threshold, retainBest against a sort, the disc against the oracle's cv::circle
and a hand-written array, and the order of suppression and mask."""
import numpy as np
import pytest

import fast_ref as F

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]


def segment_test(img, x, y, t):
    """nine contiguous ring pixels all brighter than v + t or all darker than v - t (16-bit ring masks)"""
    v = int(img[y, x])
    br = dk = 0
    for k, (dx, dy) in enumerate(RING):
        p = int(img[y + dy, x + dx])
        br |= (p > v + t) << k
        dk |= (p < v - t) << k
    for m in (br | (br << 16), dk | (dk << 16)):
        if any(((m >> s) & 0x1FF) == 0x1FF for s in range(16)):
            return True
    return False


@pytest.mark.parametrize("threshold", [7, 20, 60])
def test_score_is_the_largest_passing_threshold(oracle, threshold):
    rng = np.random.default_rng(threshold)
    # noise of limited depth on a few flat levels: plenty of corners and plenty of non-corners at every threshold
    img = (rng.integers(0, 3, (40, 48)) * 100 + rng.integers(0, 30, (40, 48))).astype(np.uint8)
    s = F.score_plane(img, threshold)
    ncorner = 0
    for _ in range(300):
        x, y = int(rng.integers(3, 45)), int(rng.integers(3, 37))
        if not segment_test(img, x, y, threshold):
            assert s[y, x] == 0, (x, y)
            continue
        best = max(t for t in range(threshold, 256) if segment_test(img, x, y, t))
        assert s[y, x] == best and threshold <= best <= 254, (x, y)
        ncorner += 1
    assert ncorner >= 20
    assert not s[:3].any() and not s[-3:].any() and not s[:, :3].any() and not s[:, -3:].any()


@pytest.mark.parametrize("resp", [[9, 5, 7, 7, 3, 7, 8], [4, 4, 4, 4], [200, 1, 1, 50, 50, 49, 51], [10]])
@pytest.mark.parametrize("n_best", [-1, 0, 1, 2, 3, 4, 5, 300])
def test_retain_best_by_sorting(resp, n_best):
    keep = F.retain_best(resp, n_best)
    r = np.asarray(resp)
    if n_best == 0:
        want = np.zeros(len(r), bool)
    elif n_best < 0 or n_best >= len(r):
        want = np.ones(len(r), bool)
    else:
        want = r >= sorted(resp)[-n_best]
    assert np.array_equal(keep, want)
    if 0 < n_best < len(r):
        assert keep.sum() >= n_best   # ties at the boundary are all kept


def test_retain_best_ties_at_above_and_below_the_boundary():
    resp = [30, 20, 20, 20, 10, 10]
    assert F.retain_best(resp, 1).tolist() == [True, False, False, False, False, False]     # the tie lies below the boundary
    assert F.retain_best(resp, 2).tolist() == [True, True, True, True, False, False]        # at it: all three stay
    assert F.retain_best(resp, 4).tolist() == [True, True, True, True, False, False]        # above it
    assert F.retain_best(resp, 5).tolist() == [True] * 6


def test_disc_shape(oracle):
    want = np.array([[0, 0, 1, 0, 0],
                     [0, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1],
                     [0, 1, 1, 1, 0],
                     [0, 0, 1, 0, 0]], bool)
    assert F.disc_spans(2) == [0, 1, 2, 1, 0]
    assert np.array_equal(F.mask_plane(5, 5, [[2, 2]], 2), want)
    for r in (0, 1, 2, 3, 5, 16):
        for cx, cy in ((20, 20), (0, 0), (39, 1), (-1, 38)):   # inside, clipped at the corners, centre outside
            m = oracle.draw_disc(np.full((40, 40), 255, np.uint8), cx, cy, r, 0)
            assert np.array_equal(F.mask_plane(40, 40, [[cx, cy]], r), m == 0), (r, cx, cy)
    # half to even: 2.5 -> 2, 3.5 -> 4
    assert F.cv_round(2.5) == 2 and F.cv_round(3.5) == 4 and F.cv_round(-0.5) == 0
    assert np.array_equal(F.mask_plane(9, 9, [[2.5, 3.5]], 0), F.mask_plane(9, 9, [[2, 4]], 0))


def test_mask_comes_after_the_suppression(oracle):
    """two adjacent corners: the stronger one suppresses the weaker one, and masking the stronger one does not bring it back"""
    img = np.full((16, 16), 200, np.uint8)
    img[8, 8], img[8, 9] = 20, 60
    s = F.score_plane(img, 20)
    assert s[8, 8] > s[8, 9] > 0
    xy, resp = F.detect(img, 20, -1, None, -1)
    assert xy.tolist() == [[8, 8]] and resp.tolist() == [s[8, 8]]
    xy, resp = F.detect(img, 20, 0, [[8, 8]], -1)
    assert len(xy) == 0
    xy, resp = F.detect(img, 20, 0, [[8, 9]], -1)   # masking the weaker one changes nothing
    assert xy.tolist() == [[8, 8]]
