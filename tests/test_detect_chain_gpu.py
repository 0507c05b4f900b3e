"""GPU parity tests (through the C ABI) of the keyframe detector chain of ov2_detect_grid_batch_dev against the CPU
oracle, at the shapes the existing detector tests leave out: the headline cell size 13 (one-wave cell kernels), both
sides of the cell^2 = 256 thread-count boundary and the entry point's limits, batches whose images share every launch,
FAST mode on the same mask and lists, the edge cases of the mask / work-list / assembly kernels, and calls of changing
shape on one context.  Everything is compared bit for bit: counts, fp32 positions as uint32, f64 thresholds."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu

W, H = 752, 480
MINEIG, FAST = 1, 0


def _pyramid(ctx, raws):
    ims = fe.Images(ctx, len(raws), W, H)
    for b, r in enumerate(raws):
        ims.upload(b, r)
    return fe.preprocess_images(ctx, ims)      # CLAHE'd frames, as the front-end detects on


def _thinned(n, B, seed):
    base = synth.grid_keypoints(n)
    rng = np.random.default_rng(seed)
    return [base[rng.uniform(size=len(base)) < 0.85] for _ in range(B)]


def _detect(ctx, pyr, cell, mode, d_th, kps, valid=None, roi=None, subpix=True):
    """one ov2_detect_grid_batch_dev call on device-resident arguments -> list of (n_b, 2) f32 arrays"""
    B = len(kps)
    cap = 2 * (W // cell) * (H // cell)
    n_cur = int(sum(len(k) for k in kps))
    d_xy = d_img = d_val = None
    if n_cur:
        d_xy = ctx.to_device(np.concatenate(kps).astype(np.float32))
        d_img = ctx.to_device(np.concatenate([np.full(len(k), b, np.int32) for b, k in enumerate(kps)]))
        if valid is not None:
            d_val = ctx.to_device(np.concatenate(valid).astype(np.uint8))
    d_n = ctx.to_device(np.full(B, -7, np.int32))            # stale counts: the call must write every image's
    d_out = ctx.empty((B, cap, 2), np.float32)
    fe.detect_grid_batch_dev(ctx, pyr, cell, mode, d_th, n_cur, d_xy, d_img, d_val, d_n, d_out, cap, roi=roi, subpix=subpix)
    ctx.synchronize()
    n, out = d_n.get(), d_out.get()
    assert (n >= 0).all() and (n <= cap).all()
    return [out[b, :n[b]].copy() for b in range(B)]


def _oracle(oracle, cl, cell, mode, kps, th, roi=None, subpix=True):
    if mode == MINEIG:
        return oracle.detect_single_scale(cl, cell, kps, th, roi=roi, subpix=subpix)
    pts, t = oracle.detect_grid_fast(cl, cell, kps, int(th), roi=roi, subpix=subpix)
    return pts, float(t)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _run_and_compare(ctx, oracle, pyr, cls, cell, mode, d_th, th, kps, valid=None, roi=None, subpix=True):
    """one call against the oracle per image; th (host list) is advanced; returns the points"""
    got = _detect(ctx, pyr, cell, mode, d_th, kps, valid, roi, subpix)
    th_dev = d_th.get()
    for b, cl in enumerate(cls):
        cur = kps[b] if valid is None else kps[b][valid[b]]
        want, th[b] = _oracle(oracle, cl, cell, mode, cur, th[b], roi, subpix)
        print(f"cell {cell} mode {mode} image {b}: {len(got[b])} points (oracle {len(want)}), threshold {th_dev[b]!r} (oracle {th[b]!r})")
        assert len(got[b]) == len(want), (cell, mode, b)
        assert _same(got[b], want), (cell, mode, b)
        assert th_dev[b] == th[b], (cell, mode, b)
    return got


def test_headline_shape(ctx, oracle, stream):
    """bench.py's keyframe shape: cell 13, 2048 grid keypoints thinned to 85 %, min-eig + cornerSubPix, B = 8"""
    B, cell = 8, 13
    raws = [stream.left(3 * b) for b in range(B)]
    cls = [oracle.clahe(r) for r in raws]
    pyr = _pyramid(ctx, raws)
    kps = _thinned(2048, B, seed=5)
    d_th, th = ctx.to_device(np.full(B, 0.001)), [0.001] * B
    for kf in range(3):          # the thresholds stay on the device and adapt from keyframe to keyframe
        got = _run_and_compare(ctx, oracle, pyr, cls, cell, MINEIG, d_th, th, kps)
        assert min(len(g) for g in got) >= 300, (kf, [len(g) for g in got])


@pytest.mark.parametrize("cell", [8, 13, 16, 17, 35, 64])
def test_cell_sizes(ctx, oracle, stream, cell):
    """both thread counts, the cell^2 = 256 boundary (16 / 17) and the limits of the entry point (8, 64)"""
    raw = stream.left(0)
    cls = [oracle.clahe(raw)]
    pyr = _pyramid(ctx, [raw])
    kps = _thinned((W // cell) * (H // cell), 1, seed=cell)
    d_th, th = ctx.to_device(np.full(1, 0.001)), [0.001]
    for kf in range(3):
        got = _run_and_compare(ctx, oracle, pyr, cls, cell, MINEIG, d_th, th, kps)
        if kf == 0:
            assert len(got[0]) > 0


@pytest.mark.parametrize("cell", [35, 50])
def test_fast_mode(ctx, oracle, stream, cell):
    """detectGridFAST shares the mask (and its polarity) and the work lists; every call's points feed the next, so the
    later calls run with every list (nearly) empty"""
    raws = [stream.left(0), stream.left(3)]
    cls = [oracle.clahe(r) for r in raws]
    pyr = _pyramid(ctx, raws)
    kps = [np.zeros((0, 2), np.float32) for _ in raws]
    d_th, th = ctx.to_device(np.full(len(raws), 10.0)), [10.0] * len(raws)
    for kf in range(3):
        got = _run_and_compare(ctx, oracle, pyr, cls, cell, FAST, d_th, th, kps)
        if kf == 0:
            assert min(len(g) for g in got) > 0
        kps = [np.concatenate([k, g]) for k, g in zip(kps, got)]


def test_no_keypoints_and_single_image(ctx, oracle, stream):
    """n_cur = 0 (no mask launch, null keypoint arrays) and B = 1"""
    raw = stream.left(5)
    pyr = _pyramid(ctx, [raw])
    got = _run_and_compare(ctx, oracle, pyr, [oracle.clahe(raw)], 13, MINEIG, ctx.to_device(np.full(1, 0.001)), [0.001],
                           [np.zeros((0, 2), np.float32)])
    assert len(got[0]) >= 300


@pytest.mark.parametrize("mode,cell,th0", [(MINEIG, 8, 0.001), (MINEIG, 17, 0.001), (FAST, 17, 10.0)])
def test_first_keyframe_of_a_batch(ctx, oracle, stream, mode, cell, th0):
    """no existing keypoints, B = 8: every cell of every image is listed (11 280 / 2464 cells per colour: lists, grids
    and point counts several times what the device holds at once), on both thread counts, with and without a roi; the
    second keyframe runs on the first one's points"""
    B = 8
    raws = [stream.left(2 * b) for b in range(B)]
    cls = [oracle.clahe(r) for r in raws]
    pyr = _pyramid(ctx, raws)
    kps = [np.zeros((0, 2), np.float32) for _ in range(B)]
    d_th, th = ctx.to_device(np.full(B, th0)), [th0] * B
    for kf in range(2):
        got = _run_and_compare(ctx, oracle, pyr, cls, cell, mode, d_th, th, kps)
        if kf == 0:
            assert min(len(g) for g in got) > 0
            if mode == MINEIG and cell == 8:
                assert sum(len(g) for g in got) > 32768
        kps = [np.concatenate([k, g]) for k, g in zip(kps, got)]
    got = _run_and_compare(ctx, oracle, pyr, cls, cell, mode, ctx.to_device(np.full(B, th0)), [th0] * B,
                           [np.zeros((0, 2), np.float32) for _ in range(B)], roi=[90, 50, 560, 370])
    assert min(len(g) for g in got) > 0


@pytest.mark.parametrize("cell", [13, 35])
def test_every_cell_occupied(ctx, oracle, stream, cell):
    """a keypoint at every cell centre, the partial last row and column included: empty lists, no points, and the
    threshold stays (0 is neither below 0.33 x 0 nor above 0.9 x 0)"""
    raws = [stream.left(1), stream.left(4)]
    pyr = _pyramid(ctx, raws)
    cx = np.arange(0, W, cell) + cell // 2
    cy = np.arange(0, H, cell) + cell // 2
    g = np.stack(np.meshgrid(cx[cx < W], cy[cy < H]), -1).reshape(-1, 2).astype(np.float32)
    d_th, th = ctx.to_device(np.full(2, 0.001)), [0.001, 0.001]
    got = _run_and_compare(ctx, oracle, pyr, [oracle.clahe(r) for r in raws], cell, MINEIG, d_th, th, [g, g])
    assert all(len(x) == 0 for x in got) and th == [0.001, 0.001]


def test_border_keypoints(ctx, oracle, stream):
    """keypoints on and beyond the image border: clipped discs, the cr == nhcells / cc == nwcells occupancy entries"""
    raws = [stream.left(2), stream.left(6)]
    pyr = _pyramid(ctx, raws)
    edge = np.array([[0, 0], [751.4, 479.4], [751.6, 100.2], [300.3, 479.6], [-5, 100], [760, 200], [300, -2], [300, 485],
                     [-40, -40], [800, 500], [1.5, 478.5], [750.5, 1.5], [376, 0], [0, 240], [751, 240], [376, 479],
                     [741.2, 470.9], [745.0, 3.0]], np.float32)
    for cell in (13, 35):
        kps = [np.concatenate([edge, k]) for k in _thinned((W // cell) * (H // cell) // 2, 2, seed=11)]
        _run_and_compare(ctx, oracle, pyr, [oracle.clahe(r) for r in raws], cell, MINEIG, ctx.to_device(np.full(2, 0.001)),
                         [0.001, 0.001], kps)


def test_roi_and_validity_mask(ctx, oracle, stream):
    """a roi that cuts cells away (the arg-max passes end a cell early) and a d_cur_valid mask; min-eig at both thread
    counts and FAST"""
    B = 3
    raws = [stream.left(2 * b + 1) for b in range(B)]
    cls = [oracle.clahe(r) for r in raws]
    pyr = _pyramid(ctx, raws)
    roi = [100, 60, 500, 300]
    rng = np.random.default_rng(2)
    for mode, cell, th0 in ((MINEIG, 13, 0.001), (MINEIG, 35, 0.001), (FAST, 35, 10.0)):
        kps = _thinned((W // cell) * (H // cell), B, seed=20 + cell)
        valid = [rng.uniform(size=len(k)) < 0.7 for k in kps]
        d_th, th = ctx.to_device(np.full(B, th0)), [th0] * B
        for kf in range(2):
            got = _run_and_compare(ctx, oracle, pyr, cls, cell, mode, d_th, th, kps, valid=valid, roi=roi)
            if mode == MINEIG and kf == 0:
                assert min(len(g) for g in got) > 0
        # roi without subpix: the integer arg-max positions themselves
        _run_and_compare(ctx, oracle, pyr, cls, cell, mode, ctx.to_device(np.full(B, th0)), [th0] * B, kps, roi=roi, subpix=False)


def test_shape_changes_on_one_context(ctx, oracle, stream):
    """(B = 8, cell 13), then (B = 2, cell 50), then the first again: the scratch block is laid out per call, so the
    third result must equal the first (stale counters, lists or weights would show here)"""
    raws8 = [stream.left(b) for b in range(8)]
    pyr8, pyr2 = _pyramid(ctx, raws8), _pyramid(ctx, raws8[:2])
    kps8, kps2 = _thinned(2048, 8, seed=31), _thinned(135, 2, seed=32)

    def first():
        d_th = ctx.to_device(np.full(8, 0.001))
        return _detect(ctx, pyr8, 13, MINEIG, d_th, kps8), d_th.get()

    a, tha = first()
    for mode, th0 in ((MINEIG, 0.001), (FAST, 10.0)):
        _run_and_compare(ctx, oracle, pyr2, [oracle.clahe(r) for r in raws8[:2]], 50, mode, ctx.to_device(np.full(2, th0)),
                         [th0, th0], kps2)
    c, thc = first()
    assert min(len(x) for x in a) >= 300
    assert all(_same(x, y) for x, y in zip(a, c)) and np.array_equal(tha, thc)
    want, t = oracle.detect_single_scale(oracle.clahe(raws8[7]), 13, kps8[7], 0.001)
    assert _same(c[7], want) and thc[7] == t


@pytest.mark.parametrize("mode,cell,th0", [(MINEIG, 13, 0.001), (MINEIG, 35, 0.001), (FAST, 35, 10.0)])
def test_batch_equals_single(ctx, stream, mode, cell, th0):
    """image b of a batched call equals a one-image call on a pyramid of that image alone"""
    B = 4
    raws = [stream.left(2 * b) for b in range(B)]
    kps = _thinned((W // cell) * (H // cell), B, seed=40 + cell)
    d_th = ctx.to_device(np.full(B, th0))
    got = _detect(ctx, _pyramid(ctx, raws), cell, mode, d_th, kps)
    th = d_th.get()
    assert sum(len(g) for g in got) > 0
    for b in range(B):
        d1 = ctx.to_device(np.full(1, th0))
        one = _detect(ctx, _pyramid(ctx, [raws[b]]), cell, mode, d1, [kps[b]])
        assert _same(one[0], got[b]), b
        assert d1.get()[0] == th[b], b
