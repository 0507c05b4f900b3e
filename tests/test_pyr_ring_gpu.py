"""The pyramid pool's ring (ov2_ctx_set_pyr_ring): its depth decides how far a build may run ahead of the tracking call
that consumes it, never what is computed.  Every test runs the frame loop of bench.py's Workload.step -- left pyramid,
tracking, on every third frame right pyramid + stereo matching + detector on the side stream -- on 752 x 480 frames that
differ from one frame to the next, synchronises nothing until the end, copies every frame's outputs into slots of their
own on the device and compares them with np.array_equal against the run at depth 2: a build into a buffer that a kernel
still reads would change them.  Each test runs on a context of its own (the pool counters start at zero); the images
and keypoints live on a shared one."""
import numpy as np
import pytest

from ov2slam_amd import _lib, frontend as fe, synth

pytestmark = pytest.mark.gpu

W, H = 752, 480
WIN, NLVL = 9, 3
NPOS = 7                 # cycle of distinct frame batches: no multiple of the number of buffers any depth keeps in rotation
FRAMES, KF_EVERY = 36, 3
SHAPES = {(8, 2048): 13, (1, 64): 64, (2, 256): 37}      # (images, keypoints per image) -> detector cell (8 .. 64)


@pytest.fixture(scope="module")
def host_frames(stream):
    return [stream.left(3 * t) for t in range(NPOS)], [stream.right(3 * t) for t in range(NPOS)]


@pytest.fixture(scope="module")
def dctx():
    """owns the inputs every run reads"""
    c = fe.Context(0)
    yield c
    c.close()


@pytest.fixture()
def rctx():
    """the context under test: fresh, so its pool is empty and its counters are zero"""
    made = []

    def make():
        made.append(fe.Context(0))
        return made[-1]
    yield make
    for c in made:
        c.close()


class Inputs:
    """device-resident inputs of the loop for B images x kps keypoints: per cycle position the image batches and the
    tracking priors; keypoints, stereo priors and the detector's existing keypoints are the same at every position"""

    def __init__(self, ctx, stream, frames, B, kps):
        left, right = frames
        self.B, self.kps, self.n, self.cell = B, kps, B * kps, SHAPES[(B, kps)]
        base = synth.grid_keypoints(kps, seed=11)
        self.left, self.right, self.pri, self.has = [], [], [], []
        for c in range(NPOS):
            il, ir = fe.Images(ctx, B, W, H), fe.Images(ctx, B, W, H)
            pri, has = [], []
            for b in range(B):
                cur, prv = (c + b) % NPOS, (c - 1 + b) % NPOS
                il.upload(b, left[cur])
                ir.upload(b, right[cur])
                p, h = synth.make_priors(base, stream.flow(3 * prv, 3 * cur, base), sigma=1.0, seed=100 + 31 * c + b)
                pri.append(p); has.append(h)
            self.left.append(il); self.right.append(ir)
            self.pri.append(ctx.to_device(np.concatenate(pri).astype(np.float32)))
            self.has.append(ctx.to_device(np.concatenate(has).astype(np.uint8)))
        sp, sh = zip(*[synth.make_priors(base, stream.stereo_gt(base), sigma=1.0, seed=13 + b) for b in range(B)])
        self.d_kps = ctx.to_device(np.concatenate([base] * B).astype(np.float32))
        self.d_spri = ctx.to_device(np.concatenate(sp).astype(np.float32))
        self.d_shas = ctx.to_device(np.concatenate(sh).astype(np.uint8))
        self.d_img = ctx.to_device(np.repeat(np.arange(B, dtype=np.int32), kps))
        rng = np.random.default_rng(5)
        cells = synth.grid_keypoints((W // self.cell) * (H // self.cell), seed=9)   # 85 % of the cells hold a keypoint
        cur = [cells[rng.uniform(size=len(cells)) < 0.85] for _ in range(B)]
        self.n_cur = int(sum(len(c) for c in cur))
        self.d_cur = ctx.to_device(np.concatenate(cur).astype(np.float32))
        self.d_cur_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(cur)]))
        self.cap = 2 * (W // self.cell) * (H // self.cell)


_inputs = {}


@pytest.fixture(scope="module")
def inputs(dctx, stream, host_frames):
    def get(B, kps):
        if (B, kps) not in _inputs:
            _inputs[(B, kps)] = Inputs(dctx, stream, host_frames, B, kps)
        return _inputs[(B, kps)]
    yield get
    _inputs.clear()


def run_loop(ctx, d, depth=None, mctx=None):
    """FRAMES frames of Workload.step at ring depth `depth` (None: as the context stands); with `mctx` the keyframe's right
    pyramid and stereo matching run on that second context, which retains the left pyramid and releases it with
    release_from (bench.py --mapper-ctx 1; no detector there).  Returns ({name: array per frame}, pool counters)."""
    if depth is not None:
        ctx.set_pyr_ring(depth)
        if mctx is not None:
            mctx.set_pyr_ring(depth)
    n, B = d.n, d.B
    sctx = mctx or ctx                                  # where the stereo call runs
    trk, strk = fe.FeatureTracker(ctx, 30, 0.01), fe.FeatureTracker(sctx, 30, 0.01)
    live = dict(xy=ctx.to_device(np.zeros((n, 2), np.float32)), st=ctx.to_device(np.zeros(n, np.uint8)),
                p3p=ctx.to_device(np.zeros(B, np.int32)),
                rxy=sctx.to_device(np.zeros((n, 2), np.float32)), rst=sctx.to_device(np.zeros(n, np.uint8)),
                th=ctx.to_device(np.full(B, 0.001, np.float64)), nout=ctx.to_device(np.full(B, -7, np.int32)),
                corners=ctx.to_device(np.zeros((B, d.cap, 2), np.float32)))
    per_frame, per_kf = ("xy", "st", "p3p"), ("rxy", "rst") + (() if mctx else ("th", "nout", "corners"))
    kfs = [t for t in range(FRAMES) if t % KF_EVERY == 0]
    slots = {k: {t: live[k].ctx.empty(live[k].shape, live[k].dtype) for t in (kfs if k in per_kf else range(1, FRAMES))}
             for k in per_frame + per_kf}              # allocated up front: an allocation synchronises
    prev = None
    for t in range(FRAMES):
        c = t % NPOS
        cur = fe.preprocess_images(ctx, d.left[c], True, 3.0, WIN, NLVL)
        if prev is not None:
            trk.kltTracking_dev(prev, cur, WIN, NLVL, 30.0, 0.5, d.d_kps, d.pri[c], d.has[c], live["xy"], live["st"], n,
                                d.d_img, live["p3p"], None)
            prev.release()
            for k in per_frame:
                slots[k][t].copy_from(live[k])
        prev = cur
        if t % KF_EVERY:
            continue
        left = cur.retain() if mctx else cur
        rp = fe.preprocess_images(sctx, d.right[c], True, 3.0, WIN, NLVL)
        strk.stereoMatching_dev(left, rp, WIN, NLVL, 30.0, 0.5, d.d_kps, d.d_spri, d.d_shas, live["rxy"], live["rst"], n,
                                d.d_img, None, True, None)
        rp.release()
        if mctx:
            left.release_from(mctx)
        else:
            fe.detect_grid_batch_dev(ctx, cur, d.cell, 1, live["th"], d.n_cur, d.d_cur, d.d_cur_img, None, live["nout"],
                                     live["corners"], d.cap)
        for k in per_kf:
            slots[k][t].copy_from(live[k])
    prev.release()
    ctx.synchronize()
    if mctx:
        mctx.synchronize()
    return {k: [slots[k][t].get() for t in sorted(slots[k])] for k in slots}, ctx.pyr_pool_stats()


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        for t, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k, t)


_ref = {}


def reference(key, make_ctx, d, mapper=False):
    """the run at depth 2 (the pool as it was before the ring had a depth), computed once per shape"""
    if key not in _ref:
        res, _ = run_loop(make_ctx(), d, 2, make_ctx() if mapper else None)
        assert sum(int(s.sum()) for s in res["st"]) > 0 and sum(int(s.sum()) for s in res["rst"]) > 0
        if not mapper:
            assert all((c > 0).all() for c in res["nout"])
        assert any(not np.array_equal(res["xy"][0], x) for x in res["xy"][1:])     # the frames do differ
        _ref[key] = res
    return _ref[key]


@pytest.mark.parametrize("B,kps", [(8, 2048), (1, 64)])
def test_loop_equals_depth_two(rctx, inputs, B, kps):
    """depths 1, 2, 3 and 6 on one context, in rising order (raising frees nothing).  At B = 8 the host runs ahead of the
    device and nearly every build takes a pending buffer; at B = 1 with 64 keypoints the device comes closer to keeping up
    and more builds find a finished one (3 / 5 / 16 of 48 at depths 2 / 3 / 6 when this was written; the counts are printed)."""
    d = inputs(B, kps)
    ref = reference((B, kps), rctx, d)
    ctx = rctx()
    before = ctx.pyr_pool_stats()
    assert before == dict(alive=0, pooled=0, finished=0, pending=0, allocated=0)
    for depth in (1, 2, 3, 6):
        res, st = run_loop(ctx, d, depth)
        served = {k: st[k] - before[k] for k in ("finished", "pending", "allocated")}
        print(f"B {B} kps {kps} depth {depth}: alive {st['alive']} pooled {st['pooled']}, builds served by finished / pending / new "
              f"buffers {served['finished']} / {served['pending']} / {served['allocated']}")
        assert_same(ref, res, (B, kps, depth))
        # the loop holds prev, cur and the right pyramid; the pool adds at most `depth` pending ones before it reuses
        assert st["alive"] <= 3 + depth and st["pooled"] == st["alive"]
        assert sum(served.values()) == FRAMES + len(range(0, FRAMES, KF_EVERY))
        if depth == 1:
            assert st["allocated"] <= 4
        before = st


def test_lowering_the_depth_frees_buffers(rctx, inputs):
    d = inputs(8, 2048)
    ref = reference((8, 2048), rctx, d)
    ctx = rctx()
    res, st6 = run_loop(ctx, d, 6)
    assert_same(ref, res, "depth 6")
    ctx.set_pyr_ring(2)
    st = ctx.pyr_pool_stats()
    print(f"depth 6 -> 2: alive {st6['alive']} -> {st['alive']}, pooled {st6['pooled']} -> {st['pooled']}")
    assert st["pooled"] <= 2 and st["alive"] == st["pooled"] and st["alive"] <= st6["alive"]
    res, st = run_loop(ctx, d)
    assert_same(ref, res, "depth 2 after 6")
    assert st["alive"] <= 3 + 2


def test_second_context_consumer(rctx, inputs):
    """the keyframe's left pyramid retained for a consumer on another context and released with release_from: the next
    build into that buffer waits for the foreign readers at every depth"""
    d = inputs(2, 256)
    ref = reference("mapper", rctx, d, mapper=True)
    res, st = run_loop(rctx(), d, 4, rctx())
    assert_same(ref, res, "second context, depth 4")
    assert st["alive"] <= 3 + 4


def test_argument_checks(rctx, inputs):
    d = inputs(1, 64)
    ctx = rctx()
    ctx.set_pyr_ring(3)
    _, st = run_loop(ctx, d)
    for bad in (0, 9, -1):
        with pytest.raises(_lib.Ov2Error, match=r"invalid argument \(-1\)"):
            ctx.set_pyr_ring(bad)
        assert ctx.lib.ov2_ctx_set_pyr_ring(ctx.h, bad) == -1      # OV2_ERR_INVALID
        assert ctx.pyr_pool_stats() == st                          # nothing was freed: the depth is still 3
    ref = reference((1, 64), rctx, d)
    res, st = run_loop(ctx, d)
    assert_same(ref, res, "after refused depths")
    assert st["alive"] <= 3 + 3
