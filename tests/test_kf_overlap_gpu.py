"""The keyframe detector chain on the side stream, beside the stereo matching of the same keyframe
(ov2_ctx_set_kf_overlap): every result must be the one the serial order gives.  Each test runs the same calls with the
overlap off and on, on one context, and compares statuses, right positions, corner counts, corners and thresholds with
np.array_equal: the headline pair at two batch sizes and in both detector modes, 60 repetitions on pooled pyramids
with nothing synchronised in between, the hazard cases that must fall back to the serial order, shapes that make both
scratch blocks grow in mid-sequence, and a run with kernel timing on."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu

W, H = 752, 480
WIN, NLVL = 9, 3
MINEIG, FAST = 1, 0
KPS = 2048
SHAPES = {MINEIG: (13, 0.001), FAST: (35, 10.0)}     # detector mode -> (cell, first threshold)


@pytest.fixture(scope="module")
def kctx():
    """a context of its own: the tests switch the overlap of the context they run on"""
    c = fe.Context(0)
    yield c
    c.close()


def _images(ctx, raws):
    ims = fe.Images(ctx, len(raws), W, H)
    for b, r in enumerate(raws):
        ims.upload(b, r)
    return ims


class Keyframe:
    """device-resident arguments of one stereo-matching + detector pair on B images"""

    def __init__(self, ctx, stream, B, mode, seed=0):
        self.ctx, self.B, self.mode = ctx, B, mode
        self.cell, self.th0 = SHAPES[mode]
        base = synth.grid_keypoints(KPS, seed=seed + 7)
        pri, has = zip(*[synth.make_priors(base, stream.stereo_gt(base), sigma=1.0, seed=seed + 13 + b) for b in range(B)])
        self.n = B * KPS
        self.kps_host = np.concatenate([base] * B).astype(np.float32)
        self.d_kps = ctx.to_device(self.kps_host)
        self.d_pri = ctx.to_device(np.concatenate(pri).astype(np.float32))
        self.d_has = ctx.to_device(np.concatenate(has).astype(np.uint8))
        self.d_img = ctx.to_device(np.repeat(np.arange(B, dtype=np.int32), KPS))
        rng = np.random.default_rng(seed + 5)
        cells = synth.grid_keypoints((W // self.cell) * (H // self.cell), seed=seed + 9)   # 85 % of the cells hold a keypoint
        cur = [cells[rng.uniform(size=len(cells)) < 0.85] for _ in range(B)]
        self.cur_host = np.concatenate(cur).astype(np.float32)
        self.n_cur = len(self.cur_host)
        self.d_cur = ctx.to_device(self.cur_host)
        self.d_cur_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(cur)]))
        self.cap = 2 * (W // self.cell) * (H // self.cell)
        self.trk = fe.FeatureTracker(ctx, 30, 0.01)
        self.fresh()

    def fresh(self):
        """outputs and detector state as before the first keyframe"""
        ctx = self.ctx
        self.d_rxy = ctx.to_device(np.zeros((self.n, 2), np.float32))
        self.d_rst = ctx.to_device(np.zeros(self.n, np.uint8))
        self.d_th = ctx.to_device(np.full(self.B, self.th0, np.float64))
        self.d_nout = ctx.to_device(np.full(self.B, -7, np.int32))
        self.d_out = ctx.to_device(np.zeros((self.B, self.cap, 2), np.float32))

    def stereo(self, left, right, d_kps=None):
        self.trk.stereoMatching_dev(left, right, WIN, NLVL, 30.0, 0.5, self.d_kps if d_kps is None else d_kps, self.d_pri,
                                    self.d_has, self.d_rxy, self.d_rst, self.n, self.d_img, None, True, None)

    def detect(self, pyr, d_cur=None, n_cur=None, d_cur_img=None, d_valid=None, d_out=None):
        fe.detect_grid_batch_dev(self.ctx, pyr, self.cell, self.mode, self.d_th, self.n_cur if n_cur is None else n_cur,
                                 self.d_cur if d_cur is None else d_cur, self.d_cur_img if d_cur_img is None else d_cur_img,
                                 d_valid, self.d_nout, self.d_out if d_out is None else d_out, self.cap)

    def results(self):
        self.ctx.synchronize()
        return dict(status=self.d_rst.get(), rxy=self.d_rxy.get().view(np.uint32), count=self.d_nout.get(),
                    corners=self.d_out.get().view(np.uint32), thresh=self.d_th.get())


def _equal(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _both_ways(ctx, run):
    """run() with the overlap off, then on: the two results"""
    out = []
    for on in (False, True):
        ctx.set_kf_overlap(on)
        try:
            out.append(run())
        finally:
            ctx.set_kf_overlap(True)
    return out


@pytest.mark.parametrize("mode", [MINEIG, FAST])
@pytest.mark.parametrize("B", [8, 64])
def test_pair_equals_serial(kctx, stream, B, mode):
    """left + right pyramid, stereo matching, detector: B x 2048 keypoints, two keyframes so that the adapted
    thresholds feed the second"""
    ctx = kctx
    left = fe.preprocess_images(ctx, _images(ctx, [stream.left(3 * (b % 8)) for b in range(B)]), True, 3.0, WIN, NLVL)
    right = fe.preprocess_images(ctx, _images(ctx, [stream.right(3 * (b % 8)) for b in range(B)]), True, 3.0, WIN, NLVL)
    kf = Keyframe(ctx, stream, B, mode)

    def run():
        kf.fresh()
        res = []
        for _ in range(2):
            kf.stereo(left, right)
            kf.detect(left)
            res.append(kf.results())
        return res

    off, on = _both_ways(ctx, run)
    for k, (a, b) in enumerate(zip(off, on)):
        print(f"B {B} mode {mode} keyframe {k}: {int(a['status'].sum())} stereo matches, {int(a['count'].sum())} corners")
        assert a["status"].sum() > 0 and a["count"].sum() > 0
        _equal(a, b, (B, mode, k))


def test_sixty_keyframes_on_pooled_pyramids(kctx, stream):
    """the loop of bench.py's Workload.step with every frame a keyframe: pyramids come from and go back to the pool,
    tracking runs between the keyframes, and nothing is synchronised until the end -- each repetition's outputs are
    copied into slots of their own on the device.  Events, both scratch blocks and the tracking counters are reused
    60 times in flight."""
    ctx, B, REPS = kctx, 8, 60
    L = [_images(ctx, [stream.left(3 * ((c + b) % 5)) for b in range(B)]) for c in range(4)]
    R = [_images(ctx, [stream.right(3 * ((c + b) % 5)) for b in range(B)]) for c in range(4)]
    kf = Keyframe(ctx, stream, B, MINEIG)
    d_trk_xy, d_trk_st = ctx.empty((kf.n, 2), np.float32), ctx.empty((kf.n,), np.uint8)
    d_p3p = ctx.empty((B,), np.int32)
    names = ("d_rst", "d_rxy", "d_nout", "d_out", "d_th")

    def run():
        kf.fresh()
        slots = [[ctx.empty(getattr(kf, n).shape, getattr(kf, n).dtype) for n in names] for _ in range(REPS)]
        prev = None
        for rep in range(REPS):
            c = rep % 4
            cur = fe.preprocess_images(ctx, L[c], True, 3.0, WIN, NLVL)
            if prev is not None:
                kf.trk.kltTracking_dev(prev, cur, WIN, NLVL, 30.0, 0.5, kf.d_kps, kf.d_pri, kf.d_has, d_trk_xy, d_trk_st, kf.n,
                                       kf.d_img, d_p3p, None)
                prev.release()
            prev = cur
            rp = fe.preprocess_images(ctx, R[c], True, 3.0, WIN, NLVL)
            kf.stereo(cur, rp)
            rp.release()
            kf.detect(cur)
            for s, n in zip(slots[rep], names):
                s.copy_from(getattr(kf, n))
        prev.release()
        ctx.synchronize()
        return [[s.get() for s in sl] for sl in slots]

    off, on = _both_ways(ctx, run)
    assert all((a[2] > 0).all() for a in off)
    for rep, (a, b) in enumerate(zip(off, on)):
        for n, x, y in zip(names, a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (rep, n)


def _pyramids(ctx, stream, B):
    left = fe.preprocess_images(ctx, _images(ctx, [stream.left(3 * b) for b in range(B)]), True, 3.0, WIN, NLVL)
    right = fe.preprocess_images(ctx, _images(ctx, [stream.right(3 * b) for b in range(B)]), True, 3.0, WIN, NLVL)
    return left, right


def test_hazard_detector_reads_the_stereo_output(kctx, stream):
    """d_cur_xy / d_cur_valid of the detector are the arrays the stereo call writes: the chain must wait for it"""
    ctx, B = kctx, 8
    left, right = _pyramids(ctx, stream, B)
    kf = Keyframe(ctx, stream, B, MINEIG)

    def run():
        kf.fresh()
        kf.stereo(left, right)
        kf.detect(left, d_cur=kf.d_rxy, n_cur=kf.n, d_cur_img=kf.d_img, d_valid=kf.d_rst)
        return kf.results()

    off, on = _both_ways(ctx, run)
    assert off["status"].sum() > 0 and (off["count"] > 0).all()
    _equal(off, on)


def test_hazard_detector_writes_the_stereo_input(kctx, stream):
    """d_out_xy of the detector covers the keypoint array the stereo call reads (the corners of image 0 land on the
    first keypoints): the chain must wait for it"""
    ctx, B = kctx, 8
    left, right = _pyramids(ctx, stream, B)
    kf = Keyframe(ctx, stream, B, MINEIG)
    assert B * kf.cap * 8 >= kf.kps_host.nbytes
    block = ctx.empty((B, kf.cap, 2), np.float32)
    as_kps = C.c_void_p(block.ptr.value)

    def run():
        kf.fresh()
        host = np.zeros((B * kf.cap, 2), np.float32)
        host[:kf.n] = kf.kps_host
        block.set(host.reshape(B, kf.cap, 2))
        kf.stereo(left, right, d_kps=as_kps)
        kf.detect(left, d_out=block)
        res = kf.results()
        res["corners"] = block.get().view(np.uint32)
        return res

    off, on = _both_ways(ctx, run)
    assert off["status"].sum() > 0 and (off["count"] > 0).all()
    assert not np.array_equal(off["corners"].reshape(-1, 2)[:8], kf.kps_host.view(np.uint32)[:8])   # they did land there
    _equal(off, on)


@pytest.mark.parametrize("between", ["copy", "tracking"])
def test_hazard_call_between_the_two(kctx, stream, between):
    """another call enqueued between the stereo call and the detector: a device copy that replaces the detector's
    keypoints (the detector must see the new ones), or a tracking call"""
    ctx, B = kctx, 8
    left, right = _pyramids(ctx, stream, B)
    kf = Keyframe(ctx, stream, B, MINEIG)
    rng = np.random.default_rng(3)
    moved = (kf.cur_host + rng.uniform(-40, 40, kf.cur_host.shape)).astype(np.float32)
    d_moved = ctx.to_device(moved)
    d_trk_xy, d_trk_st, d_p3p = ctx.empty((kf.n, 2), np.float32), ctx.empty((kf.n,), np.uint8), ctx.empty((B,), np.int32)

    def run(with_between=True):
        kf.fresh()
        kf.d_cur.set(kf.cur_host)
        kf.stereo(left, right)
        if with_between and between == "copy":
            kf.d_cur.copy_from(d_moved)
        elif with_between:
            kf.trk.kltTracking_dev(left, right, WIN, NLVL, 30.0, 0.5, kf.d_kps, kf.d_pri, kf.d_has, d_trk_xy, d_trk_st, kf.n,
                                   kf.d_img, d_p3p, None)
        kf.detect(left)
        return kf.results()

    off, on = _both_ways(ctx, run)
    assert (off["count"] > 0).all()
    _equal(off, on, between)
    if between == "copy":
        ctx.set_kf_overlap(False)
        try:
            plain = run(with_between=False)
        finally:
            ctx.set_kf_overlap(True)
        assert not np.array_equal(plain["corners"], off["corners"])   # the copy does change what the detector finds


def test_shapes_that_grow_both_scratch_blocks(stream):
    """8, then 64, then 8 images on a fresh context: both scratch blocks grow at the first and at the second shape, with
    the other stream's work in flight"""
    ctx = fe.Context(0)
    try:
        pyr = {B: _pyramids(ctx, stream, B) if B == 8 else
               (fe.preprocess_images(ctx, _images(ctx, [stream.left(3 * (b % 8)) for b in range(B)]), True, 3.0, WIN, NLVL),
                fe.preprocess_images(ctx, _images(ctx, [stream.right(3 * (b % 8)) for b in range(B)]), True, 3.0, WIN, NLVL))
               for B in (8, 64)}
        kfs = {B: Keyframe(ctx, stream, B, MINEIG) for B in (8, 64)}

        def run():
            res = []
            for B in (8, 64, 8):
                kf = kfs[B]
                kf.fresh()
                kf.stereo(*pyr[B])
                kf.detect(pyr[B][0])
                res.append(kf.results())
            return res

        ctx.set_kf_overlap(True)
        on = run()
        ctx.set_kf_overlap(False)
        off = run()
        for k, (a, b) in enumerate(zip(off, on)):
            assert (a["count"] > 0).all()
            _equal(a, b, k)
        _equal(on[0], on[2], "first and third shape")
    finally:
        ctx.close()


def test_with_kernel_timing(kctx, stream):
    """ctx.kernel_timing(True) brackets every launch with events on the stream it runs on"""
    ctx, B = kctx, 8
    left, right = _pyramids(ctx, stream, B)
    kf = Keyframe(ctx, stream, B, MINEIG)

    def run():
        kf.fresh()
        ctx.kernel_timing(True)
        try:
            kf.stereo(left, right)
            kf.detect(left)
            res = kf.results()
            times = ctx.kernel_times()
        finally:
            ctx.kernel_timing(False)
        assert times["subpix_kernel"][1] == 1 and times["detect_cell_kernels"][1] == 4 and times["klt_stage2_kernel"][1] == 1
        assert all(t >= 0.0 for t, _ in times.values())
        return res

    off, on = _both_ways(ctx, run)
    _equal(off, on)
