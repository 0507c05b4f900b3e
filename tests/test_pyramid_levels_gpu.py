"""GPU parity of the two-level pyrDown launch (level l -> l+1 -> l+2 in one kernel, one workgroup per 32 x 16 px tile of
level l+2 with the level-(l+1) ring recomputed).  Builds step by two levels per launch and run pyrdown_kernel for a level
left over, so every depth from 3 to 6 levels is covered, on the CLAHE path (two-level steps from level 1) and on the
plain-copy path (from level 0).  Ragged sizes give partial last tiles, level-(l+2) tiles one column or row wide and
levels narrower than one tile; windows 5 .. 15 put the pad on both sides of the 6-px reach of the staged level.
Bar: bit-exact against the CPU oracle, padded REFLECT_101 borders and gradient planes included."""
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


def _oracle_pyr(oracle, img, use_clahe, win, nl, tiles):
    src = oracle.clahe(img, 3.0, tiles[0], tiles[1]) if use_clahe else img
    return oracle.Pyramid(src, win, nl)


# EuRoC geometry at 3 .. 6 levels: one two-level step, one step + a single level, two steps, two steps + a single level
@pytest.mark.parametrize("use_clahe", [True, False])
@pytest.mark.parametrize("nl", [2, 3, 4, 5])
def test_levels_euroc_depths(ctx, oracle, use_clahe, nl):
    img = synth.StereoStream().left(3)
    gp = fe.preprocess_image(ctx, img, use_clahe=use_clahe, klt_win_size=9, nklt_pyr_lvl=nl)
    assert gp.nlevels == nl + 1
    _assert_pyr_equal(gp, _oracle_pyr(oracle, img, use_clahe, 9, nl, fe.clahe_tiles(752, 480)))


# 257 / 259 px: a level-(l+2) tile one column wide on the CLAHE path (level 2 = 65 px = 2 x 32 + 1), 130 x 66 the same
# on the plain path; 389 x 241 ragged in both directions; 133 x 61 levels narrower than one tile
@pytest.mark.parametrize("w,h", [(257, 61), (259, 131), (130, 66), (389, 241), (133, 61)])
@pytest.mark.parametrize("win", [5, 9, 11, 15])
@pytest.mark.parametrize("use_clahe", [True, False])
def test_levels_ragged(ctx, oracle, w, h, win, use_clahe):
    img = _image(w, h, 17 * w + h + win)
    tiles = (max(w // 50, 1), max(h // 50, 1))
    gp = fe.preprocess_image(ctx, img, use_clahe=use_clahe, fclahe_val=3.0, klt_win_size=win, nklt_pyr_lvl=5, tiles=tiles)
    _assert_pyr_equal(gp, _oracle_pyr(oracle, img, use_clahe, win, 5, tiles))


@pytest.mark.parametrize("use_clahe", [True, False])
def test_levels_batch_per_image(ctx, oracle, use_clahe):
    S = synth.StereoStream()
    raw = [S.left(1), S.right(4), _image(752, 480, 9), np.full((480, 752), 201, np.uint8), S.left(6)]
    ims = fe.Images(ctx, len(raw), 752, 480)
    for b, im in enumerate(raw):
        ims.upload(b, im)
    gp = fe.preprocess_images(ctx, ims, use_clahe, 3.0, 9, 4)
    ctx.synchronize()
    assert gp.batch == len(raw)
    for b, im in enumerate(raw):
        _assert_pyr_equal(gp, _oracle_pyr(oracle, im, use_clahe, 9, 4, fe.clahe_tiles(752, 480)), b)
