"""GPU parity of the fused CLAHE + level-0 + first-pyrDown kernel on the tile classes its 128 x 60 px workgroups create:
ragged last block columns and row bands, the window sizes that move the reflected border across tiles, CLAHE tile grids
that make a block touch the most interpolation cells the fused path admits, every pyramid depth, and a batch of distinct
images.  Bar: bit-exact against the CPU oracle, padded REFLECT_101 borders and gradient planes included."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu


def _assert_pyr_equal(gp, op, b=0):
    assert gp.nlevels == op.nlevels
    for l in range(op.nlevels):
        gi, gg, w, h, p = gp.level(l, b)
        oi, og, ow, oh, opad = op.level(l)
        assert (w, h, p) == (ow, oh, opad)
        assert np.array_equal(gi, oi), f"image {b} level {l} differs at {np.argwhere(gi != oi)[:5]}"
        assert np.array_equal(gg, og), f"image {b} level {l} gradient differs at {np.argwhere(gg != og)[:5]}"


def _image(w, h, seed):
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0, 255, w)[None, :] * 0.5 + np.linspace(0, 60, h)[:, None]
    return (ramp + rng.integers(0, 128, size=(h, w))).clip(0, 255).astype(np.uint8)


# last block column 1, 3, 5, 7 px wide (w mod 128) and a last row band of 1 row (h mod 60 == 1) or a full one
@pytest.mark.parametrize("w,h", [(257, 61), (259, 121), (261, 181), (263, 120), (133, 61), (389, 241)])
@pytest.mark.parametrize("win", [5, 9, 11, 15])
def test_fused_ragged_tiles(ctx, oracle, w, h, win):
    img = _image(w, h, 31 * w + h + win)
    tiles = (max(w // 50, 1), max(h // 50, 1))
    gp = fe.preprocess_image(ctx, img, use_clahe=True, fclahe_val=3.0, klt_win_size=win, nklt_pyr_lvl=3, tiles=tiles)
    _assert_pyr_equal(gp, oracle.Pyramid(oracle.clahe(img, 3.0, tiles[0], tiles[1]), win, 3))


# 24 x 16 px and 24 x 17 px CLAHE tiles: a block touches up to 8 x 6 / 8 x 5 interpolation cells (the fused path admits 51)
@pytest.mark.parametrize("w,h,tiles", [(192, 128, (8, 8)), (261, 181, (11, 11))])
@pytest.mark.parametrize("nl", [0, 1, 2, 3])
def test_fused_many_cells(ctx, oracle, w, h, tiles, nl):
    img = _image(w, h, w + 7 * h)
    gp = fe.preprocess_image(ctx, img, use_clahe=True, fclahe_val=2.0, klt_win_size=9, nklt_pyr_lvl=nl, tiles=tiles)
    _assert_pyr_equal(gp, oracle.Pyramid(oracle.clahe(img, 2.0, tiles[0], tiles[1]), 9, nl))


@pytest.mark.parametrize("nl", [0, 1, 2, 3])
@pytest.mark.parametrize("win", [9, 15])
def test_fused_euroc_levels(ctx, oracle, nl, win):
    img = synth.StereoStream().left(2)
    gp = fe.preprocess_image(ctx, img, use_clahe=True, klt_win_size=win, nklt_pyr_lvl=nl)
    _assert_pyr_equal(gp, oracle.Pyramid(oracle.clahe(img), win, nl))


def test_fused_batch_per_image(ctx, oracle):
    S = synth.StereoStream()
    raw = [S.left(1), S.right(4), _image(752, 480, 5), np.full((480, 752), 17, np.uint8)]
    ims = fe.Images(ctx, len(raw), 752, 480)
    for b, im in enumerate(raw):
        ims.upload(b, im)
    gp = fe.preprocess_images(ctx, ims, True, 3.0, 11, 3)
    ctx.synchronize()
    assert gp.batch == len(raw)
    for b, im in enumerate(raw):
        _assert_pyr_equal(gp, oracle.Pyramid(oracle.clahe(im), 11, 3), b)
