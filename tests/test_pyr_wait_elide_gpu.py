"""Waits for pyramids that the main stream does not need (ov2_pyr_wait_ready, ov2_pyr_need_grad, ov2_ctx_pyr_wait_stats).

The owner context's main stream waits for a build once; later calls on the same pyramid enqueue no event packet, and a
build that has already completed needs none either.  A consumer on another context always waits.  The frame loop is
bench.py's Workload.step as tests/test_pyr_ring_gpu.py runs it (left pyramid, tracking, on every third frame right
pyramid + stereo matching + the detector on the side stream), here on 2 images x 256 keypoints and 13 frames.  The loop
that synchronises nothing must give the outputs of the same loop synchronised after every call, array for array, and the
counters must add up:

  calls           every tracking call asks for prev and cur, the stereo call for left and right, the detector for its
                  pyramid; with 8 lanes per keypoint the tracking and stereo calls ask for the gradient planes of both too;
  issued          event waits enqueued;
  found_complete  requests left out because the event had completed when asked for;
  elided          every request that was left out: found_complete + the requests for a build already waited for.
  For the pyramids a context builds and consumes itself, issued + found_complete == builds EXACTLY: every build is waited
  for, or found complete, once, at its first request -- a library that skips a wait it needs shows fewer, one that repeats
  a wait shows more.  Which of the two a first request turns out to be depends on how far the host runs ahead, so the
  loops assert the sum; test_build_not_complete_when_asked_for holds the builds back behind work the device provably has
  not finished and asserts issued == builds, and the synchronised loop asserts found_complete == builds.
"""
import numpy as np
import pytest

import test_pyr_ring_gpu as R
from test_pyr_ring_gpu import dctx, host_frames, inputs, rctx  # noqa: F401  (fixtures)
from ov2slam_amd import frontend as fe

pytestmark = pytest.mark.gpu

FRAMES, KF_EVERY = 13, 3
B, KPS = 2, 256
KFS = [t for t in range(FRAMES) if t % KF_EVERY == 0]


def run_loop(ctx, d, depth, mctx=None, sync=False, lanes=3):
    """R.run_loop with a switch that synchronises after every call, a forced lane mapping and the wait counters of both
    contexts.  Returns ({name: array per frame}, wait stats of ctx, wait stats of mctx or None)."""
    ctx.set_pyr_ring(depth)
    ctx.set_klt_lanes(lanes)
    if mctx is not None:
        mctx.set_pyr_ring(depth)
        mctx.set_klt_lanes(lanes)
    n = d.n
    sctx = mctx or ctx

    def settle():
        if sync:
            ctx.synchronize()
            if mctx is not None:
                mctx.synchronize()
    trk, strk = fe.FeatureTracker(ctx, 30, 0.01), fe.FeatureTracker(sctx, 30, 0.01)
    live = dict(xy=ctx.to_device(np.zeros((n, 2), np.float32)), st=ctx.to_device(np.zeros(n, np.uint8)),
                p3p=ctx.to_device(np.zeros(d.B, np.int32)),
                rxy=sctx.to_device(np.zeros((n, 2), np.float32)), rst=sctx.to_device(np.zeros(n, np.uint8)),
                th=ctx.to_device(np.full(d.B, 0.001, np.float64)), nout=ctx.to_device(np.full(d.B, -7, np.int32)),
                corners=ctx.to_device(np.zeros((d.B, d.cap, 2), np.float32)))
    per_frame, per_kf = ("xy", "st", "p3p"), ("rxy", "rst") + (() if mctx else ("th", "nout", "corners"))
    slots = {k: {t: live[k].ctx.empty(live[k].shape, live[k].dtype) for t in (KFS if k in per_kf else range(1, FRAMES))}
             for k in per_frame + per_kf}              # allocated up front: an allocation synchronises
    ctx.synchronize()
    sctx.synchronize()
    w0, m0 = ctx.pyr_wait_stats(), (mctx.pyr_wait_stats() if mctx else None)
    prev = None
    for t in range(FRAMES):
        c = t % R.NPOS
        cur = fe.preprocess_images(ctx, d.left[c], True, 3.0, R.WIN, R.NLVL)
        settle()
        if prev is not None:
            trk.kltTracking_dev(prev, cur, R.WIN, R.NLVL, 30.0, 0.5, d.d_kps, d.pri[c], d.has[c], live["xy"], live["st"], n,
                                d.d_img, live["p3p"], None)
            prev.release()
            for k in per_frame:
                slots[k][t].copy_from(live[k])
            settle()
        prev = cur
        if t % KF_EVERY:
            continue
        left = cur.retain() if mctx else cur
        rp = fe.preprocess_images(sctx, d.right[c], True, 3.0, R.WIN, R.NLVL)
        settle()
        strk.stereoMatching_dev(left, rp, R.WIN, R.NLVL, 30.0, 0.5, d.d_kps, d.d_spri, d.d_shas, live["rxy"], live["rst"], n,
                                d.d_img, None, True, None)
        rp.release()
        settle()
        if mctx:
            left.release_from(mctx)
        else:
            fe.detect_grid_batch_dev(ctx, cur, d.cell, 1, live["th"], d.n_cur, d.d_cur, d.d_cur_img, None, live["nout"],
                                     live["corners"], d.cap)
        for k in per_kf:
            slots[k][t].copy_from(live[k])
        settle()
    prev.release()
    ctx.synchronize()
    if mctx:
        mctx.synchronize()
    diff = lambda a, b: {k: a[k] - b[k] for k in a}
    return ({k: [slots[k][t].get() for t in sorted(slots[k])] for k in slots}, diff(ctx.pyr_wait_stats(), w0),
            diff(mctx.pyr_wait_stats(), m0) if mctx else None)


def expected(mapper, lanes):
    """(calls, builds consumed) of the owner context and of the second one, per the module docstring"""
    per = 1 if lanes == 3 else 2                  # 8 / 16 lanes: every pyramid is also asked for its gradient planes
    K, T = len(KFS), FRAMES
    if not mapper:
        return (per * 2 * (T - 1) + per * 2 * K + K, T + K), None
    # second context: the stereo call alone; `left` is foreign there (always waited for), `right` is its own build
    return (per * 2 * (T - 1), T), (per * 2 * K, K)


_ref = {}


def synchronised(key, make_ctx, d, mapper, lanes):
    """the loop synchronised after every call, once per (contexts, lanes): the outputs every other run must equal.  Every
    build has completed when a call asks for it, so no wait is issued by a context for its own pyramids."""
    if key not in _ref:
        res, w, m = run_loop(make_ctx(), d, 3, make_ctx() if mapper else None, sync=True, lanes=lanes)
        (calls, builds), second = expected(mapper, lanes)
        print(f"synchronised {key}: owner {w}, second context {m}")
        assert w == dict(issued=0, elided=calls, found_complete=builds)
        if mapper:   # the foreign `left` waited for at every call, its own `right` found complete
            assert m == dict(issued=len(KFS), elided=len(KFS), found_complete=len(KFS))
        assert sum(int(s.sum()) for s in res["st"]) > 0 and sum(int(s.sum()) for s in res["rst"]) > 0
        assert any(not np.array_equal(res["xy"][0], x) for x in res["xy"][1:])     # the frames do differ
        _ref[key] = res
    return _ref[key]


@pytest.mark.parametrize("mapper", [False, True], ids=["one_ctx", "second_ctx"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_unsynchronised_loop(rctx, inputs, depth, mapper):
    d = inputs(B, KPS)
    ref = synchronised(("sync", mapper, 3), rctx, d, mapper, 3)
    res, w, m = run_loop(rctx(), d, depth, rctx() if mapper else None)
    (calls, builds), second = expected(mapper, 3)
    print(f"depth {depth} second context {mapper}: owner {w} of {calls} calls on {builds} builds, second context {m}")
    R.assert_same(ref, res, (depth, mapper))
    assert w["issued"] + w["elided"] == calls
    assert w["issued"] + w["found_complete"] == builds     # every build waited for or found complete, once
    if mapper:
        # its own `right` pyramids once each (waited for or found complete), the foreign `left` waited for at every call
        assert m["issued"] + m["elided"] == second[0]
        assert m["issued"] + m["found_complete"] == 2 * second[1] and m["elided"] == m["found_complete"] <= second[1]


def test_gradient_planes_follow_the_rule(rctx, inputs):
    """8 lanes per keypoint: the tracking kernels read the Scharr planes, written on the consumer's main stream behind the
    build.  The owner wrote them on the stream that reads them, so no call waits for grad_ev either."""
    d = inputs(B, KPS)
    ref = synchronised(("sync", False, 8), rctx, d, False, 8)
    res, w, _ = run_loop(rctx(), d, 3, lanes=8)
    (calls, builds), _ = expected(False, 8)
    print(f"8 lanes: owner {w} of {calls} calls on {builds} builds")
    R.assert_same(ref, res, "8 lanes")
    assert w["issued"] + w["elided"] == calls
    assert w["issued"] + w["found_complete"] == builds     # no grad_ev is asked for: the planes are the stream's own


def test_foreign_context_always_waits(rctx, inputs):
    """both pyramids built on one context and complete, the stereo call made three times on another: every call waits for
    both (an elision there would need a record of what a foreign stream has seen), and computes what the owner computes"""
    d = inputs(B, KPS)
    ctx, other = rctx(), rctx()
    left = fe.preprocess_images(ctx, d.left[0], True, 3.0, R.WIN, R.NLVL)
    right = fe.preprocess_images(ctx, d.right[0], True, 3.0, R.WIN, R.NLVL)
    ctx.synchronize()
    out = {}
    for name, c in (("owner", ctx), ("other", other)):
        c.set_klt_lanes(3)
        trk = fe.FeatureTracker(c, 30, 0.01)
        xy, st = c.to_device(np.zeros((d.n, 2), np.float32)), c.to_device(np.zeros(d.n, np.uint8))
        for _ in range(3):
            trk.stereoMatching_dev(left, right, R.WIN, R.NLVL, 30.0, 0.5, d.d_kps, d.d_spri, d.d_shas, xy, st, d.n, d.d_img, None,
                                   True, None)
        c.synchronize()
        out[name] = (xy.get(), st.get())
    assert ctx.pyr_wait_stats() == dict(issued=0, elided=6, found_complete=2)
    assert other.pyr_wait_stats() == dict(issued=6, elided=0, found_complete=0)
    assert int(out["owner"][1].sum()) > 0
    assert np.array_equal(out["owner"][0].view(np.uint32), out["other"][0].view(np.uint32)) and np.array_equal(out["owner"][1], out["other"][1])
    left.release()
    right.release()


def test_build_not_complete_when_asked_for(rctx, inputs):
    """Ring depth 1.  Behind 200 device-to-device copies of 128 MiB the main stream gets three release marks: first that of
    a witness pyramid of another geometry (one level fewer), then those of two pyramids of the loop's geometry.  The next
    two builds of that geometry take the two buffers and wait for their marks, so they cannot complete before the
    witness's mark has.  The stereo call on them is enqueued at once; AFTER it a build of the witness's geometry asks the
    pool for the witness's buffer, and the pool counts it as taken with its readers pending: the witness's mark had not
    completed then, so neither build had when it was asked for.  Both requests must be issued as waits, and a second call
    on the same pyramids must issue none; its outputs equal those of a third call made after a synchronise."""
    d = inputs(B, KPS)
    ctx = rctx()
    ctx.set_pyr_ring(1)
    ctx.set_klt_lanes(3)
    trk = fe.FeatureTracker(ctx, 30, 0.01)
    out = [(ctx.to_device(np.zeros((d.n, 2), np.float32)), ctx.to_device(np.zeros(d.n, np.uint8))) for _ in range(3)]
    big = [ctx.to_device(np.zeros(1 << 27, np.uint8)) for _ in range(2)]
    witness = fe.preprocess_images(ctx, d.left[0], True, 3.0, R.WIN, R.NLVL - 1)
    a = [fe.preprocess_images(ctx, im[0], True, 3.0, R.WIN, R.NLVL) for im in (d.left, d.right)]

    def stereo(left, right, o):
        trk.stereoMatching_dev(left, right, R.WIN, R.NLVL, 30.0, 0.5, d.d_kps, d.d_spri, d.d_shas, o[0], o[1], d.n, d.d_img, None,
                               True, None)
    stereo(a[0], a[1], out[0])      # the context's scratch and counters exist from here on: an allocation synchronises
    ctx.synchronize()
    p0, w0 = ctx.pyr_pool_stats(), ctx.pyr_wait_stats()
    for _ in range(200):
        big[1].copy_from(big[0])
    witness.release()
    for p in a:
        p.release()
    b = [fe.preprocess_images(ctx, im[1], True, 3.0, R.WIN, R.NLVL) for im in (d.left, d.right)]
    stereo(b[0], b[1], out[0])
    w1 = ctx.pyr_wait_stats()
    again = fe.preprocess_images(ctx, d.left[0], True, 3.0, R.WIN, R.NLVL - 1)      # the pool queries the witness's mark
    p1 = ctx.pyr_pool_stats()
    stereo(b[0], b[1], out[1])
    w2 = ctx.pyr_wait_stats()
    ctx.synchronize()
    stereo(b[0], b[1], out[2])
    ctx.synchronize()
    diff = lambda x, y: {k: x[k] - y[k] for k in x}
    print(f"pool {diff(p1, p0)}, waits of the first call {diff(w1, w0)}, of the second {diff(w2, w1)}")
    # all three builds took a buffer whose release mark had not completed: the witness's was asked after the stereo call
    assert diff(p1, p0) == dict(alive=0, pooled=0, finished=0, pending=3, allocated=0), \
        "the device had finished the copies before the witness was asked for: the case proves nothing"
    assert diff(w1, w0) == dict(issued=2, elided=0, found_complete=0)
    assert diff(w2, w1) == dict(issued=0, elided=2, found_complete=0)
    assert int(out[2][1].get().sum()) > 0
    for k in range(2):
        assert np.array_equal(out[k][0].get().view(np.uint32), out[2][0].get().view(np.uint32))
        assert np.array_equal(out[k][1].get(), out[2][1].get())
    for p in b + [again]:
        p.release()
