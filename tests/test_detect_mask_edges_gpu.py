"""The detector chain's mask at the places where a packed mask would differ from a byte per pixel (ov2slam_amd/csrc/detect.hip;
written with the one-bit-per-pixel mask of DESIGN.md section 7, "Shorter serial kernels per frame", which was measured and
left out -- the cases hold for any layout of the mask and are what a next attempt has to pass).  Small images whose rows do
and do not end on a multiple of 32 pixels, existing keypoints whose discs cross the 32-pixel boundaries, touch the first
and last column and lie partly or wholly outside the image, a batch with interleaved image indices and marks in the last
rows of an image (a disc that left its plane would mask cells of the next image), two neighbouring cells of different
colours where the earlier cell's discs cover the later cell's unmasked maximum, second candidates beside the first disc,
both modes (FAST reads the mask at a quarter of the column), a roi with validity flags, and cell sizes on both sides of
the one-wave cell kernel (8 and 13, 35).  Every case: corners
(float32 bit patterns), counts and thresholds equal the oracle's."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe

pytestmark = pytest.mark.gpu

H = 75
MINEIG, FAST = 1, 0
TH0 = {MINEIG: 0.001, FAST: 10.0}


def _crop(stream, t, w, h=H, x0=200, y0=150):
    return np.ascontiguousarray(stream.left(t)[y0:y0 + h, x0:x0 + w])


def _run(ctx, oracle, raws, cell, mode, kps, valid=None, roi=None, subpix=True, order=None, th0=None):
    """one ov2_detect_grid_batch_dev call on the images `raws` (no CLAHE) against the oracle per image; `order` permutes
    the concatenated keypoints, so the image indices arrive interleaved.  Returns the points per image"""
    B, (h, w) = len(raws), raws[0].shape
    ims = fe.Images(ctx, B, w, h)
    for b, r in enumerate(raws):
        ims.upload(b, r)
    pyr = fe.preprocess_images(ctx, ims, use_clahe=False)
    cap = 2 * (w // cell) * (h // cell)
    th0 = TH0[mode] if th0 is None else th0
    xy = np.concatenate(kps).astype(np.float32).reshape(-1, 2)
    img = np.concatenate([np.full(len(k), b, np.int32) for b, k in enumerate(kps)])
    val = None if valid is None else np.concatenate(valid).astype(np.uint8)
    if order is not None:
        xy, img = xy[order], img[order]
        val = None if val is None else val[order]
    n_cur = len(xy)
    d_xy = ctx.to_device(np.ascontiguousarray(xy)) if n_cur else None
    d_img = ctx.to_device(np.ascontiguousarray(img)) if n_cur else None
    d_val = ctx.to_device(np.ascontiguousarray(val)) if n_cur and val is not None else None
    d_th = ctx.to_device(np.full(B, th0, np.float64))
    d_n, d_out = ctx.to_device(np.full(B, -7, np.int32)), ctx.empty((B, cap, 2), np.float32)
    fe.detect_grid_batch_dev(ctx, pyr, cell, mode, d_th, n_cur, d_xy, d_img, d_val, d_n, d_out, cap, roi=roi, subpix=subpix)
    ctx.synchronize()
    n, out, th = d_n.get(), d_out.get(), d_th.get()
    got = []
    for b, raw in enumerate(raws):
        cur = np.asarray(kps[b], np.float32).reshape(-1, 2)
        if valid is not None:
            cur = cur[np.asarray(valid[b], bool)]
        if mode == MINEIG:
            want, t = oracle.detect_single_scale(raw, cell, cur, th0, roi=roi, subpix=subpix)
        else:
            want, t = oracle.detect_grid_fast(raw, cell, cur, int(th0), roi=roi, subpix=subpix)
        what = (w, cell, mode, b)
        assert 0 <= n[b] <= cap, what
        assert n[b] == len(want), what
        assert np.array_equal(out[b, :n[b]].view(np.uint32), want.view(np.uint32)), what
        assert th[b] == float(t), what
        got.append(out[b, :n[b]].copy())
    return got


def _edge_keypoints(w, h, r):
    """discs across the 32-pixel word boundaries, touching column 0 and column w - 1 from inside, cut by every border and
    wholly outside the image"""
    xs = [31.6, 30.0, 33.2, 32.0 - r, 32.0 + r, 63.0, 64.4, 0.0, float(r), w - 1.0, w - 1.0 - r, -1.0, w + 1.0, float(-r),
          w - 1.0 + r, -r - 1.0, -r - 6.0, w + r + 2.0]
    pts = [(x, 9.0 + 7.0 * (k % 8)) for k, x in enumerate(xs)]
    pts += [(20.0, -2.0), (40.3, h + 1.0), (50.0, h + r + 3.0), (10.0, -r - 1.0), (45.0, 0.0), (12.0, h - 1.0), (-2.0, -2.0),
            (w + 1.0, h + 1.0)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("cell", [8, 13, 35])
@pytest.mark.parametrize("w", [64, 65, 95, 97])
def test_widths_and_edge_discs(ctx, oracle, stream, w, cell):
    raw = _crop(stream, 0, w)
    rng = np.random.default_rng(w + cell)
    inner = np.stack([rng.uniform(0, w, 12), rng.uniform(0, H, 12)], 1).astype(np.float32)
    kps = np.concatenate([_edge_keypoints(w, H, cell // 4), inner])
    found = 0
    for mode in (MINEIG, FAST):
        found += len(_run(ctx, oracle, [raw], cell, mode, [kps])[0])
        found += len(_run(ctx, oracle, [raw], cell, mode, [np.zeros((0, 2), np.float32)], subpix=False)[0])
    assert found > 0


@pytest.mark.parametrize("mode,cell", [(MINEIG, 8), (MINEIG, 13), (FAST, 13)])
def test_batch_of_three_interleaved(ctx, oracle, stream, mode, cell):
    """three images, keypoint order shuffled over the images; images 0 and 1 carry discs in their last rows and images 1
    and 2 none in their first rows, so a disc that left its plane would mask cells of the next image"""
    w, r = 97, cell // 4
    raws = [_crop(stream, t, w, x0=180 + 40 * t) for t in range(3)]
    rng = np.random.default_rng(cell)
    kps = []
    for b in range(3):
        k = np.stack([rng.uniform(0, w, 10), rng.uniform(2 * cell, H, 10)], 1).astype(np.float32)
        if b < 2:
            last = np.stack([np.arange(3, w, 2 * r + 1, dtype=np.float32), np.full(len(range(3, w, 2 * r + 1)), H - 1.0, np.float32)], 1)
            k = np.concatenate([k, last])
        kps.append(k)
    order = rng.permutation(sum(len(k) for k in kps))
    got = _run(ctx, oracle, raws, cell, mode, kps, order=order)
    assert sum(len(g) for g in got) > 0


def _interacting_cells(cell=13):
    """a flat image with a bright bar across the border of cells (0, 0) and (0, 1) and a weaker mark inside cell (0, 1)"""
    img = np.full((H, 97), 100, np.uint8)
    img[4:10, cell - 1:cell + 2] = 255
    img[8:11, cell + 7:cell + 10] = 140
    return img


def test_neighbour_cells_of_different_colours(ctx, oracle):
    """cell (0, 0) (colour 0) runs a launch before cell (0, 1) (colour 1) and its two discs reach over the cell border,
    within 32 pixels of the row start: the later cell must see them.  The CPU side shows first that the case is live: the later
    cell's arg-max with and without the earlier cell's discs differ"""
    cell, r = 13, 3
    img = _interacting_cells(cell)
    h0, h1 = oracle.min_eig_cell(img, 0, 0, cell), oracle.min_eig_cell(img, cell, 0, cell)
    mask = np.zeros(img.shape, np.uint8)
    for _ in range(2):                                   # first and second candidate of the earlier cell
        v = np.where(mask[:cell, :cell] != 0, np.float32(0), h0)
        i = int(np.argmax(v))
        assert v.flat[i] >= 0.001
        oracle.draw_disc(mask, i % cell, i // cell, r, 1)
    free = int(np.argmax(h1))
    masked = int(np.argmax(np.where(mask[:cell, cell:2 * cell] != 0, np.float32(0), h1)))
    assert mask[:cell, cell:2 * cell].flat[free] != 0 and masked != free
    want, _ = oracle.detect_single_scale(img, cell, np.zeros((0, 2), np.float32), 0.001, subpix=False)
    assert [cell + masked % cell, masked // cell] in want.astype(int).tolist()
    assert [cell + free % cell, free // cell] not in want.astype(int).tolist()
    for subpix in (False, True):
        _run(ctx, oracle, [img], cell, MINEIG, [np.zeros((0, 2), np.float32)], subpix=subpix)


@pytest.mark.parametrize("mode,cell", [(MINEIG, 8), (MINEIG, 13), (MINEIG, 35), (FAST, 35)])
def test_roi_and_validity_flags(ctx, oracle, stream, mode, cell):
    w = 95
    raws = [_crop(stream, t, w) for t in (1, 4)]
    rng = np.random.default_rng(3 * cell)
    kps = [np.concatenate([_edge_keypoints(w, H, cell // 4), np.stack([rng.uniform(0, w, 9), rng.uniform(0, H, 9)], 1).astype(np.float32)])
           for _ in raws]
    valid = [rng.uniform(size=len(k)) < 0.6 for k in kps]
    _run(ctx, oracle, raws, cell, mode, kps, valid=valid, roi=[9, 6, 70, 55])
    _run(ctx, oracle, raws, cell, mode, kps, valid=valid, roi=[9, 6, 70, 55], subpix=False)


def test_second_candidates_beside_the_first_disc(ctx, oracle, stream):
    """no existing keypoints: every cell is free and the second arg-max of a cell runs on the cell's copy of the mask with
    the first candidate's disc in it; the oracle's point list carries the second candidates behind the first ones"""
    for cell in (8, 13, 35):
        raw = _crop(stream, 2, 97)
        got = _run(ctx, oracle, [raw], cell, MINEIG, [np.zeros((0, 2), np.float32)], subpix=False)[0]
        assert len(got) > 0
