"""Checker for ov2_fast_detect_batch: a numpy restatement of what the loop closer asks of OpenCV (src/loop_closer.cpp:95-126):
FAST_t<16> with non-maximum suppression, KeyPointsFilter::runByPixelsMask, KeyPointsFilter::retainBest, in row-major order.
Building blocks from the oracle: fast_score (cornerScore<16>), nothing of the library under test."""
import functools

import numpy as np

from oracle import oracle_py as O


@functools.lru_cache(maxsize=64)
def _score_plane(buf, w, h, threshold):
    img = np.frombuffer(buf, np.uint8).reshape(h, w)
    s = np.zeros((h, w), np.uint8)
    if w < 7 or h < 7:
        return s
    # nine contiguous ring pixels hold at least two of the four compass ones: pixels that fail that are no corners, the others
    # get the oracle's cornerScore<16> (which is 0 for those that fail the full test)
    c = img[3:h - 3, 3:w - 3].astype(np.int32)
    compass = [img[6:h, 3:w - 3], img[0:h - 6, 3:w - 3], img[3:h - 3, 6:w], img[3:h - 3, 0:w - 6]]
    brighter = sum((p.astype(np.int32) > c + threshold).astype(np.int32) for p in compass)
    darker = sum((p.astype(np.int32) < c - threshold).astype(np.int32) for p in compass)
    for y, x in zip(*np.nonzero((brighter >= 2) | (darker >= 2))):
        s[y + 3, x + 3] = O.fast_score(img, int(x) + 3, int(y) + 3, threshold)
    s.setflags(write=False)
    return s


def score_plane(img, threshold):
    """s(x, y) for 3 <= x < w-3, 3 <= y < h-3, else 0; threshold clamped to 0..255 (read-only, shared between tests)"""
    img = np.ascontiguousarray(img, np.uint8)
    return _score_plane(img.tobytes(), img.shape[1], img.shape[0], int(min(max(threshold, 0), 255)))


def nms_plane(score):
    """keypoint iff s > 0 and s strictly greater than the eight neighbours' s (outside the plane: 0)"""
    h, w = score.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = score
    c = p[1:-1, 1:-1]
    keep = c > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy != 1 or dx != 1:
                keep &= c > p[dy:dy + h, dx:dx + w]
    return keep


def disc_spans(radius):
    """half-width per row offset -radius .. radius of cv::circle(.., radius, .., FILLED) (drawing.cpp Circle()); -1: no span"""
    hw = [-1] * (2 * radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        for row, half in ((dy, dx), (dx, dy)):
            hw[radius + row] = max(hw[radius + row], half)
            hw[radius - row] = max(hw[radius - row], half)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def cv_round(v):
    """cvRound of a float: round half to even"""
    return int(np.rint(np.float32(v)))


def mask_plane(w, h, pts, radius):
    """True where masked: the union of the discs around (cvRound(x), cvRound(y)), clipped to the image"""
    m = np.zeros((h, w), bool)
    if radius < 0 or pts is None:
        return m
    hw = disc_spans(radius)
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        cx, cy = cv_round(x), cv_round(y)
        for row, half in enumerate(hw):
            yy = cy + row - radius
            if half < 0 or yy < 0 or yy >= h:
                continue
            xa, xb = max(cx - half, 0), min(cx + half, w - 1)
            if xa <= xb:
                m[yy, xa:xb + 1] = True
    return m


def retain_best(resp, n_best):
    """bool per keypoint: KeyPointsFilter::retainBest by the 256-bin histogram rule"""
    resp = np.asarray(resp, np.int64)
    if n_best < 0 or len(resp) <= n_best:
        return np.ones(len(resp), bool)
    if n_best == 0:
        return np.zeros(len(resp), bool)
    hist = np.bincount(resp, minlength=256)
    suffix = np.cumsum(hist[::-1])[::-1]              # suffix[t] = keypoints of response >= t
    bound = int(np.flatnonzero(suffix >= n_best).max())
    return resp >= bound


def detect(img, threshold, mask_radius, mask_pts, n_best):
    """-> (xy (n, 2) f32, resp (n,) u8), row-major"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    s = score_plane(img, threshold)
    kp = nms_plane(s) & ~mask_plane(w, h, mask_pts, mask_radius)   # the mask comes after the suppression
    ys, xs = np.nonzero(kp)                                        # row-major
    resp = s[ys, xs]
    keep = retain_best(resp, n_best)
    return np.stack([xs[keep], ys[keep]], axis=1).astype(np.float32).reshape(-1, 2), resp[keep].astype(np.uint8)


def expected(img, threshold, mask_radius, mask_pts, n_best, out_cap):
    """what the call writes for one image: n_total, n_out, the first n_out keypoints and responses"""
    xy, resp = detect(img, threshold, mask_radius, mask_pts, n_best)
    n = min(len(xy), out_cap)
    return len(xy), n, xy[:n], resp[:n]
