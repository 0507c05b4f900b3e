"""ov2_fast_detect_batch(_dev) on the GPU, through the C ABI, against tests/fast_ref.py: counts, positions and responses
compared with array_equal (everything is integer arithmetic).  Sizes around the 64 x 16 tile of the score pass and the dword
pitch of the planes, dense and sparse content, ties at the retainBest bound, truncation, masks with half-integer, clipped and
on-keypoint points, batches against single calls, the device-resident form and the refusals."""
import ctypes as C

import numpy as np
import pytest

import fast_ref as F

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16                      # FD_TW x FD_TH of ov2slam_amd/csrc/fastnms.hip
ONE_TILE_PLUS_ONE = (TILE_W + 1, TILE_H + 1)  # a second tile of one pixel in each direction
SIZES = [(96, 80), (101, 77), (7, 7), (6, 9), ONE_TILE_PLUS_ONE]
vp = C.c_void_p


@pytest.fixture(scope="module")
def fe():
    from ov2slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def S():
    from ov2slam_amd import synth_fast
    return synth_fast


def raw_pyramid(fe, ctx, imgs):
    """level 0 of the raw images, no CLAHE, one pyramid for the batch"""
    h, w = imgs[0].shape
    if len(imgs) == 1:
        return fe.preprocess_image(ctx, imgs[0], use_clahe=False, klt_win_size=3, nklt_pyr_lvl=0)
    im = fe.Images(ctx, len(imgs), w, h)
    for b, a in enumerate(imgs):
        im.upload(b, a)
    return fe.preprocess_images(ctx, im, use_clahe=False, klt_win_size=3, nklt_pyr_lvl=0)


def run(fe, ctx, imgs, threshold, mask_radius, masks, n_best, out_cap):
    pyr = raw_pyramid(fe, ctx, imgs)
    try:
        return fe.fast_detect_batch(ctx, pyr, threshold, mask_radius, masks, n_best, out_cap)
    finally:
        pyr.release()


def check(got, imgs, threshold, mask_radius, masks, n_best, out_cap, what=""):
    n_total, n_out, xy, resp = got
    for b, img in enumerate(imgs):
        et, eo, exy, er = F.expected(img, threshold, mask_radius, None if masks is None else masks[b], n_best, out_cap)
        assert (n_total[b], n_out[b]) == (et, eo), f"{what} image {b}: counts {n_total[b]}, {n_out[b]} != {et}, {eo}"
        assert np.array_equal(xy[b, :eo], exy), f"{what} image {b}: positions differ"
        assert np.array_equal(resp[b, :eo], er), f"{what} image {b}: responses differ"
        assert not xy[b, eo:].any() and not resp[b, eo:].any(), f"{what} image {b}: written beyond n_out"
    return n_total


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("threshold", [7, 20, 60])
def test_noise_every_size_and_threshold(fe, S, ctx, size, threshold):
    img = S.noise_image(*size, seed=size[0] * 100 + size[1])
    n = check(run(fe, ctx, [img], threshold, -1, None, -1, 4096), [img], threshold, -1, None, -1, 4096)
    if min(size) > 16 and threshold < 60:
        assert n[0] > 20   # dense corners: every tile edge carries comparisons


ROWS_MANY_FROM = 8192   # FD_ROWS_MANY_FROM: image rows in a call from which a workgroup takes 16 rows instead of 4


@pytest.mark.parametrize("h", [ROWS_MANY_FROM - 1, ROWS_MANY_FROM + 5])
def test_rows_per_workgroup_on_both_sides_of_the_switch(fe, S, ctx, h):
    """narrow and tall: the suppression, count and emit passes below and above the switch, the last workgroup partly filled"""
    img = S.noise_image(12, h, seed=h)
    pts = S.mask_points(12, h, 200, seed=2)
    for n_best, cap in ((-1, 8192), (300, 128)):
        n = check(run(fe, ctx, [img], 20, 2, [pts], n_best, cap), [img], 20, 2, [pts], n_best, cap)
        assert n[0] >= 300   # thousands without retainBest; with it the 300 and the ties at the bound


def test_one_scorable_pixel_and_none(fe, S, ctx):
    img = S.dots_image(7, 7, [(3, 3)])
    n = check(run(fe, ctx, [img], 20, -1, None, -1, 8), [img], 20, -1, None, -1, 8)
    assert n[0] == 1
    img = S.dots_image(6, 9, [(3, 4)])
    n = check(run(fe, ctx, [img], 20, -1, None, -1, 8), [img], 20, -1, None, -1, 8)
    assert n[0] == 0


@pytest.mark.parametrize("n_best", [-1, 0, 1, 300])
def test_blocks_constant_and_retain_best(fe, S, ctx, n_best):
    blocks = S.blocks_image(101, 77, seed=5)
    n = check(run(fe, ctx, [blocks], 7, -1, None, n_best, 1024), [blocks], 7, -1, None, n_best, 1024, "blocks")
    assert n[0] == 0 if n_best == 0 else n[0] >= 1
    noise = S.noise_image(101, 77, seed=6)   # more than 300 keypoints: the bound cuts through a response's ties
    assert F.expected(noise, 7, -1, None, -1, 0)[0] > 300
    check(run(fe, ctx, [noise], 7, -1, None, n_best, 2048), [noise], 7, -1, None, n_best, 2048, "noise")
    flat = S.constant_image(96, 80)
    n = check(run(fe, ctx, [flat], 20, -1, None, n_best, 16), [flat], 20, -1, None, n_best, 16, "constant")
    assert n[0] == 0


def test_blocks_image_has_isolated_corners(S):
    assert 12 <= F.expected(S.blocks_image(101, 77, seed=5), 7, -1, None, -1, 0)[0] <= 100


def test_ties_and_truncation(fe, S, ctx):
    img = S.motif_image(21, 20)   # 420 keypoints of one response
    n_total, n_out, xy, resp = got = run(fe, ctx, [img], 20, -1, None, 300, 64)
    check(got, [img], 20, -1, None, 300, 64)
    assert n_total[0] == 420 > 300 and n_out[0] == 64 and len(set(resp[0].tolist())) == 1
    assert np.array_equal(xy[0, :3], [[6, 6], [18, 6], [30, 6]])   # the first of the row-major order
    n_total, n_out, _, _ = run(fe, ctx, [img], 20, -1, None, 300, 0)
    assert (n_total[0], n_out[0]) == (420, 0)


def mask_cases(img, threshold):
    h, w = img.shape
    xy, resp = F.detect(img, threshold, -1, None, -1)
    strongest = xy[int(np.argmax(resp))]
    pts = [[10.5, 20.5], [11.5, 21.5], [30.5, 40], [31.5, 41],          # x.5 with x even and odd: half to even
           [0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1],              # clipped discs
           [-1.2, 30], [w + 0.4, 12], [1e9, -1e9],                      # centres outside the image
           strongest.tolist()] + xy[::7].tolist()                       # on top of keypoints
    return np.asarray(pts, np.float32), strongest


@pytest.mark.parametrize("mask_radius", [-1, 0, 2, 16])
@pytest.mark.parametrize("threshold", [7, 20])
def test_masks(fe, S, ctx, mask_radius, threshold):
    img = S.noise_image(101, 77, seed=9)
    pts, strongest = mask_cases(img, threshold)
    if mask_radius > 2:
        pts = pts[:12]   # the largest discs: a dozen of them leave most of the image free
    n_total, n_out, xy, _ = got = run(fe, ctx, [img], threshold, mask_radius, [pts], -1, 4096)
    check(got, [img], threshold, mask_radius, [pts], -1, 4096)
    there = (xy[0, :n_out[0]] == strongest).all(1).any()
    assert there == (mask_radius < 0)
    check(run(fe, ctx, [img], threshold, mask_radius, [pts], 300, 4096), [img], threshold, mask_radius, [pts], 300, 4096, "with retainBest")
    check(run(fe, ctx, [img], threshold, mask_radius, [pts[:0]], -1, 4096), [img], threshold, -1, None, -1, 4096, "no points")


def test_keypoints_at_the_scorable_limits(fe, S, ctx):
    w, h = 70, 37
    dots = [(3, 10), (w - 4, 12), (15, 3), (20, h - 4), (3, 3), (w - 4, h - 4), (2, 20), (w - 3, 22), (30, 2), (40, h - 3)]
    img = S.dots_image(w, h, dots)
    n_total, n_out, xy, resp = got = run(fe, ctx, [img], 20, -1, None, -1, 64)
    check(got, [img], 20, -1, None, -1, 64)
    found = {tuple(int(v) for v in p) for p in xy[0, :n_out[0]]}
    assert found == set(dots[:6])   # the four that lie outside 3 <= x < w-3, 3 <= y < h-3 are no keypoints
    assert set(resp[0, :n_out[0]].tolist()) == {159}


def test_batch_equals_singles_and_dev_form(fe, S, ctx):
    w, h = 101, 77
    imgs = [S.noise_image(w, h, seed=21), S.blocks_image(w, h, seed=22), S.noise_image(w, h, seed=23)]
    masks = [mask_cases(imgs[0], 20)[0], np.zeros((0, 2), np.float32), S.mask_points(w, h, 40, seed=3)]
    cap = 256   # truncates the noise images, not the blocks image
    pyr = raw_pyramid(fe, ctx, imgs)
    try:
        got = fe.fast_detect_batch(ctx, pyr, 20, 2, masks, 300, cap)
        check(got, imgs, 20, 2, masks, 300, cap, "batch")
        assert got[0][0] > cap and got[0][1] < cap
        for b in range(3):
            one = run(fe, ctx, [imgs[b]], 20, 2, [masks[b]], 300, cap)
            for a, o in zip(got, one):
                assert np.array_equal(a[b], o[0]), f"image {b} alone differs from its place in the batch"
        # the device-resident form, twice: same bits
        xy = np.concatenate(masks)
        idx = np.concatenate([np.full(len(m), b, np.int32) for b, m in enumerate(masks)])
        order = np.random.default_rng(0).permutation(len(xy))      # the points of the images interleaved
        d_xy, d_idx = ctx.to_device(xy[order]), ctx.to_device(idx[order])
        for _ in range(2):
            d_nt, d_no = ctx.to_device(np.full(3, -1, np.int32)), ctx.to_device(np.full(3, -1, np.int32))
            d_oxy, d_or = ctx.to_device(np.zeros((3, cap, 2), np.float32)), ctx.to_device(np.zeros((3, cap), np.uint8))
            fe.fast_detect_batch_dev(ctx, pyr, 20, 2, len(xy), d_xy, d_idx, 300, cap, d_nt, d_no, d_oxy, d_or)
            ctx.synchronize()
            for a, d in zip(got, (d_nt, d_no, d_oxy, d_or)):
                assert np.array_equal(a, d.get())
    finally:
        pyr.release()


def test_invalid_arguments(fe, S, ctx):
    img = S.noise_image(96, 80, seed=1)
    pyr = raw_pyramid(fe, ctx, [img])
    try:
        lib = ctx.lib
        nt, no = np.zeros(1, np.int32), np.zeros(1, np.int32)
        xy, rs = np.zeros((1, 8, 2), np.float32), np.zeros((1, 8), np.uint8)
        P = lambda a: a.ctypes.data_as(vp)
        INVALID = lib.ov2_fast_detect_batch(None, pyr.h, 20, -1, None, None, -1, 8, P(nt), P(no), P(xy), P(rs))
        assert INVALID != 0
        assert lib.ov2_fast_detect_batch(ctx.h, pyr.h, 20, -1, None, None, -1, -1, P(nt), P(no), P(xy), P(rs)) == INVALID
        assert lib.ov2_fast_detect_batch(ctx.h, pyr.h, 20, -1, None, None, -1, 8, None, P(no), P(xy), P(rs)) == INVALID
        assert lib.ov2_fast_detect_batch(ctx.h, pyr.h, 20, 17, None, None, -1, 8, P(nt), P(no), P(xy), P(rs)) == INVALID
        assert lib.ov2_fast_detect_batch(ctx.h, None, 20, -1, None, None, -1, 8, P(nt), P(no), P(xy), P(rs)) == INVALID
        assert lib.ov2_fast_detect_batch_dev(ctx.h, pyr.h, 20, 17, 0, None, None, -1, 0, None, None, None, None) == INVALID
        assert lib.ov2_fast_detect_batch_dev(ctx.h, pyr.h, 20, 2, 0, None, None, -1, -1, None, None, None, None) == INVALID
        # and the call still works afterwards
        check(fe.fast_detect_batch(ctx, pyr, 20, -1, None, -1, 4096), [img], 20, -1, None, -1, 4096)
    finally:
        pyr.release()
