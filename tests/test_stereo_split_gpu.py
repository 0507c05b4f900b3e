"""stereoMatching's split descent (ov2slam_amd/csrc/klt.hip, ov2_klt_set_stereo_split): the first tracking launch runs the
levels nlevels .. k + 1 of list B (keypoints without a prior) beside list A and leaves a 16-byte record per keypoint, the
second launch resumes at level k behind list C (the failures of A, re-tracked on the full pyramid).  k >= the call's level
count is the unsplit call.  Every k must give what the oracle gives: positions as float32 bit patterns, status, and BOTH
halves of the work words (low 16 bits = LK iterations, high 16 bits = level passes; list-A passes in iters[i],
full-pyramid passes in iters[n + i]) -- and therefore what the unsplit call gives, bit for bit.

The expected work words come from the oracle's calcOpticalFlowPyrLK, which reports the iterations of every level: one call
for the forward pass, the gates of fbKltTracking, one call for the backward pass.  A level counts as a pass when the
template window lies inside the image, whatever happens to the search window afterwards.

Cases and helpers of the lists are those of test_stereo_lists_gpu (lists A, B and C, see there).

A search window that is outside the image at one level is outside at every finer level of a 752 x 480 pyramid (the sizes
halve exactly: x - 4 >= w implies 2 x - 4 >= 2 w, x - 4 < -9 implies 2 x - 4 < -9), so a keypoint that leaves at a coarse
level never has an iteration again; what "comes back" at the finer levels is the PASS: every pass restarts with run = act,
the template is staged, the pass is counted and the search window is found outside at iteration 0.  The hand-over record
must not carry the `run` flag of the level it left at, and the pass counts below would show it if it did."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth
from test_stereo_lists_gpu import Batch2, Call, Pools, KPW, N_EASY, W, H, WIN, NLVL

pytestmark = pytest.mark.gpu

ERR_TH, FB_TH = 30.0, 0.5
SPLITS = (0, 1, 2, 3)          # every k at NLVL = 3; k = NLVL is the unsplit call


def _fb(oracle, o0, o1, kps, pri, nl):
    """fbKltTracking (src/feature_tracker.cpp:35-137) out of the oracle's calcOpticalFlowPyrLK: (forward result, status,
    work word = LK iterations | level passes << 16, forward iterations per level, forward err)"""
    kps, pri = np.ascontiguousarray(kps, np.float32).reshape(-1, 2), np.ascontiguousarray(pri, np.float32).reshape(-1, 2)
    n = len(kps)
    if n == 0:
        return pri, np.zeros(0, bool), np.zeros(0, np.uint32), np.zeros((0, nl + 1), np.int32), np.zeros(0, np.float32)
    out, st, err, it = oracle.calc_optical_flow_pyr_lk(o0, o1, kps, pri, WIN, nl)
    ml = it.shape[1] - 1
    passes = np.zeros(n, np.int64)
    w, h = W, H
    for l in range(ml + 1):      # the template window of level l lies inside the level (lk_level's first test)
        p = np.floor(kps * np.float32(1.0 / (1 << l)) - np.float32((WIN - 1) * 0.5))
        passes += (p[:, 0] >= -WIN) & (p[:, 0] < w) & (p[:, 1] >= -WIN) & (p[:, 1] < h)
        w, h = (w + 1) // 2, (h + 1) // 2
    ok = (st != 0) & ~(err > np.float32(ERR_TH)) & (1 <= out[:, 0]) & (out[:, 0] < W - 1) & (1 <= out[:, 1]) & (out[:, 1] < H - 1)
    iters = it.sum(1).astype(np.int64)
    idx = np.flatnonzero(ok)
    if len(idx):                 # backward pass on level 0 from the keypoint itself (:113); its template is inside by the gate
        back, bst, _, bit = oracle.calc_optical_flow_pyr_lk(o1, o0, out[idx], kps[idx], WIN, 0)
        iters[idx] += bit[:, 0]
        passes[idx] += 1
        d = (kps[idx] - back).astype(np.float64)
        ok[idx] = (bst != 0) & ~(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) > FB_TH)
    return out, ok, (iters | (passes << 16)).astype(np.uint32), it, err


def _stereo_words(oracle, o0, o1, kps, pri, has, nl=NLVL):
    """the 2 n work words a stereo call must leave: two-level pass of the keypoints with a prior, full-pyramid pass of its
    failures (from the failed forward result) and of the keypoints without a prior (from `pri`)"""
    has = np.asarray(has) != 0
    wa, wf = np.zeros(len(kps), np.uint32), np.zeros(len(kps), np.uint32)
    out_a, ok_a, wa[has], _, _ = _fb(oracle, o0, o1, kps[has], pri[has], min(1, o0.nlevels - 1))
    fail = np.flatnonzero(has)[~ok_a]
    wf[fail] = _fb(oracle, o0, o1, kps[fail], out_a[~ok_a], nl)[2]
    wf[~has] = _fb(oracle, o0, o1, kps[~has], pri[~has], nl)[2]
    return wa, wf


class CallN(Call):
    def stereo_n(self, g, nl):
        """ov2_stereo_matching_dev with nl + 1 pyramid levels asked for, enqueued"""
        self.trk.stereoMatching_dev(g[0], g[1], WIN, nl, ERR_TH, FB_TH, *self.d_in, self.d_o, self.d_s, self.n, self.d_i, None,
                                    True, None, d_iters=self.d_w)
        return self


def _check(call, exp, what):
    """positions (bit patterns), status and whole work words of one finished call against (exy, est, wa, wf)"""
    exy, est, wa, wf = exp
    out, st, work = call.get()
    n = len(exy)
    assert set(np.unique(st)) <= {0, 1}, what
    assert np.array_equal(st.astype(bool), est), what
    assert np.array_equal(out.view(np.uint32), exy.view(np.uint32)), what
    assert np.array_equal(work[:n] & 0xffff, wa & 0xffff) and np.array_equal(work[n:] & 0xffff, wf & 0xffff), (what, "iterations")
    assert np.array_equal(work[:n] >> 16, wa >> 16) and np.array_equal(work[n:] >> 16, wf >> 16), (what, "passes")


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a.get(), b.get())):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


@pytest.fixture(scope="module")
def pools(ctx, oracle, stream):
    return Pools(ctx, oracle, stream, 0)


@pytest.fixture(scope="module")
def batch2(ctx, oracle, stream, pools):
    return Batch2(ctx, oracle, stream, pools)


@pytest.fixture(scope="module")
def expected(oracle, pools):
    """(kps, prior, has_prior) and (positions, status, work words) of a case of the pools, the oracle run once per shape"""
    memo = {}

    def get(nb, nc, na):
        if (nb, nc, na) not in memo:
            kps, pri, has, exy, est = pools.case(oracle, nb, nc, na)[:5]
            memo[nb, nc, na] = (kps, pri, has), (exy, est) + _stereo_words(oracle, *pools.o, kps, pri, has)
        return memo[nb, nc, na]
    return get


@pytest.fixture
def knobs(ctx):
    """(lanes per keypoint, split level) of the shared context; the defaults are put back"""
    def choose(gl, k):
        ctx.set_klt_lanes(gl)
        ctx.set_stereo_split(k)
    try:
        yield choose
    finally:
        ctx.set_klt_lanes(0)
        ctx.set_stereo_split(-1)


def test_setter(ctx):
    assert ctx.lib.ov2_klt_set_stereo_split(None, 1) == -1     # OV2_ERR_INVALID
    for k in (0, 1, 5, -1, -9):
        ctx.set_stereo_split(k)                                # any k is legal: k >= levels is no split, k < 0 the default


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_every_split_level(ctx, expected, pools, knobs, gl):
    """every k of a four-level call, more than two waves of list B and more than one of list C, and the library's own
    default: all equal to the oracle, and to the unsplit call bit for bit"""
    k = KPW[gl]
    args, exp = expected(2 * k + 1, k + 1, N_EASY)
    res = {}
    for s in (NLVL,) + SPLITS[:-1] + (NLVL + 4, -1):
        knobs(gl, s)
        res[s] = CallN(ctx, *args).stereo_n(pools.g, NLVL)
        ctx.synchronize()
        _check(res[s], exp, (gl, s))
        _same(res[s], res[NLVL], (gl, s))


@pytest.mark.parametrize("gl,nb,nc", [(gl, nb, nc) for gl in (3, 8, 16) for nb in (0, 1, KPW[gl] - 1, KPW[gl], KPW[gl] + 1, 2 * KPW[gl] + 1)
                                      for nc in (0, 1, KPW[gl] + 1)])
def test_list_lengths_around_the_wave(ctx, expected, pools, knobs, gl, nb, nc):
    args, exp = expected(nb, nc, N_EASY)
    for s in (1, 0):
        knobs(gl, s)
        got = CallN(ctx, *args).stereo_n(pools.g, NLVL)
        ctx.synchronize()
        _check(got, exp, (gl, nb, nc, s))


@pytest.mark.parametrize("gl", [3, 8, 16])
@pytest.mark.parametrize("nl", [0, 1])
def test_one_and_two_level_calls(ctx, oracle, pools, knobs, gl, nl):
    """nlevels = 0: nothing to cut; nlevels = 1: one level on either side of the only cut (k = 0)"""
    kps, pri, has = pools.case(oracle, KPW[gl] + 1, 3, N_EASY)[:3]
    exp = oracle.stereo_matching(*pools.o, kps, pri, has, nlevels=nl) + _stereo_words(oracle, *pools.o, kps, pri, has, nl)
    ref = None
    for s in (nl, 0, 1, 2, -1):
        knobs(gl, s)
        got = CallN(ctx, kps, pri, has).stereo_n(pools.g, nl)
        ctx.synchronize()
        _check(got, exp, (gl, nl, s))
        ref = ref or got
        _same(got, ref, (gl, nl, s))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_pyramid_with_fewer_levels_than_asked(ctx, oracle, pools, knobs, gl):
    """two-level pyramids and a call that asks for four: make_params clamps the call to two, so k = 1, 2, 3 are no split
    and k = 0 cuts between the two levels"""
    L, R = pools.raw
    g = fe.preprocess_image(ctx, L, use_clahe=False, nklt_pyr_lvl=1), fe.preprocess_image(ctx, R, use_clahe=False, nklt_pyr_lvl=1)
    o = oracle.Pyramid(L, WIN, 1), oracle.Pyramid(R, WIN, 1)
    assert o[0].nlevels == 2
    kps, pri, has = pools.case(oracle, KPW[gl] + 1, 3, N_EASY)[:3]
    exp = oracle.stereo_matching(*o, kps, pri, has, nlevels=NLVL) + _stereo_words(oracle, *o, kps, pri, has, NLVL)
    ref = None
    for s in (3, 2, 1, 0, -1):
        knobs(gl, s)
        got = CallN(ctx, kps, pri, has).stereo_n(g, NLVL)
        ctx.synchronize()
        _check(got, exp, (gl, s))
        ref = ref or got
        _same(got, ref, (gl, s))
    for p in g:
        p.release()


FLAT = (slice(200, 440), slice(40, 280))     # a 240 x 240 block of one grey value: 30 x 30 pixels on level 3
FLAT_KP = (160.3, 320.6)


def special_case(oracle, stream):
    """A stereo pair with a flat block painted into both images, and a list B whose first four keypoints, BY THE ORACLE,
    (0) leave the image during the iterations of the top level and are found outside at iteration 0 of every finer level,
    (1) fail the min-eigenvalue test on level 3 (and below: the block is flat on every level), (2) run all 30 iterations
    on some level above 0, (3) pass every forward gate and fail the backward pass alone; then ordinary keypoints of all
    three lists.  returns (left, right, kps, prior, has_prior)"""
    L, R = stream.left(0).copy(), stream.right(0).copy()
    L[FLAT] = 128
    R[FLAT] = 128
    o = oracle.Pyramid(L), oracle.Pyramid(R)
    rng = np.random.default_rng(1)
    xs, ys = np.meshgrid(np.arange(12, W - 12, 16), np.arange(12, H - 12, 16))
    kps = (np.stack([xs.ravel(), ys.ravel()], 1) + rng.uniform(0, 1, (xs.size, 2))).astype(np.float32)
    inside = (kps[:, 0] > FLAT[1].start - 45) & (kps[:, 0] < FLAT[1].stop + 45) & (kps[:, 1] > FLAT[0].start - 45) & (kps[:, 1] < FLAT[0].stop + 45)
    kps = kps[~inside]                       # the grid stays clear of the block on every level
    gt = stream.stereo_gt(kps).astype(np.float32)
    ang, r = rng.uniform(0, 2 * np.pi, len(kps)), rng.uniform(6.0, 10.0, len(kps))
    far = (gt + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)).astype(np.float32)
    # (0) near the right border, prior beyond it
    kb = kps[kps[:, 0] > W - 40]
    pb = kb.copy()
    pb[:, 0] = (W + rng.uniform(5, 30, len(kb))).astype(np.float32)
    out, ok, wd, it, err = _fb(oracle, *o, kb, pb, NLVL)
    p = np.floor(out - np.float32(4.0))
    gone = (p[:, 0] >= W) | (p[:, 0] < -WIN) | (p[:, 1] >= H) | (p[:, 1] < -WIN)
    c0 = np.flatnonzero(gone & (it[:, NLVL] > 0) & (it[:, :NLVL] == 0).all(1) & ~ok & (wd >> 16 == NLVL + 1))
    assert len(c0), "no candidate leaves the image on the top level"
    # (1) the middle of the flat block, prior inside it: in the image on level 3, so 0 iterations there is the eigenvalue test
    kf, pf = np.array([FLAT_KP], np.float32), np.array([[FLAT_KP[0] - 12.0, FLAT_KP[1]]], np.float32)
    _, okf, wdf, itf, errf = _fb(oracle, *o, kf, pf, NLVL)
    assert (itf == 0).all() and errf[0] < 1e-4 and not okf[0] and wdf[0] == (NLVL + 1) << 16
    # (2), (3) among the keypoints with a prior 15 - 25 px off
    r = rng.uniform(15.0, 25.0, len(kps))
    far2 = (gt + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)).astype(np.float32)
    out, ok, wd, it, err = _fb(oracle, *o, kps, far2, NLVL)
    c2 = np.flatnonzero((it[:, 1:] == 30).any(1))
    c3 = np.flatnonzero(~ok & (wd >> 16 == NLVL + 2))      # the backward pass ran: every forward gate was passed
    assert len(c2) and len(c3[c3 != c2[0]]), (len(c2), len(c3))
    i2, i3 = c2[0], c3[c3 != c2[0]][0]
    far[[i2, i3]] = far2[[i2, i3]]
    rest = np.setdiff1d(np.arange(len(kps)), [i2, i3])
    rest = rest[rng.permutation(len(rest))]
    nb, na, nc = 2 * 21 + 1 - 4, 12, 9       # list B: 43 keypoints = two three-lane waves and one keypoint
    b, a, c = rest[:nb], rest[nb:nb + na], rest[nb + na:nb + na + nc]
    K = np.concatenate([kb[c0[:1]], kf, kps[[i2, i3]], kps[b], kps[a], kps[c]])
    P = np.concatenate([pb[c0[:1]], pf, far[[i2, i3]], far[b], (gt[a] + rng.normal(0, 0.5, (na, 2))).astype(np.float32), far[c]])
    has = np.concatenate([np.zeros(4 + nb, np.uint8), np.ones(na + nc, np.uint8)])
    return L, R, o, np.ascontiguousarray(K), np.ascontiguousarray(P), has


@pytest.fixture(scope="module")
def special(ctx, oracle, stream):
    L, R, o, kps, pri, has = special_case(oracle, stream)
    g = fe.preprocess_image(ctx, L, use_clahe=False), fe.preprocess_image(ctx, R, use_clahe=False)
    exp = oracle.stereo_matching(*o, kps, pri, has) + _stereo_words(oracle, *o, kps, pri, has)
    assert (exp[3][has != 0] != 0).any() and (exp[3][has != 0] == 0).any()       # list C is there, and not all of list A
    return g, (kps, pri, has), exp


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_keypoints_that_stop_early_or_late(ctx, special, knobs, gl):
    g, args, exp = special
    ref = None
    for s in (NLVL,) + SPLITS[:-1]:
        knobs(gl, s)
        got = CallN(ctx, *args).stereo_n(g, NLVL)
        ctx.synchronize()
        _check(got, exp, (gl, s))
        ref = ref or got
        _same(got, ref, (gl, s))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_batch_of_two_interleaved(ctx, batch2, knobs, gl):
    for s in (1, 0):
        knobs(gl, s)
        got = batch2.stereo_call(ctx).stereo(batch2.g[:2])
        ctx.synchronize()
        batch2.check_stereo(got, (gl, s))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_tracking_between_stereo_calls(ctx, batch2, knobs, gl):
    """stereo, kltTracking (both outcomes of the 33 % rule), stereo: every argument on the device first, then the three calls
    enqueued with nothing synchronised in between -- the hand-over block is the same memory in both stereo calls, the
    tracking call between them takes list B in its first launch with no split, and the second stereo call's first launch
    rewrites the records behind the first call's second launch by stream order alone"""
    knobs(gl, 1)
    s1, t, s2 = batch2.stereo_call(ctx), batch2.track_call(ctx), batch2.stereo_call(ctx)
    s1.stereo(batch2.g[:2])
    t.track((batch2.g[0], batch2.g[2]))
    s2.stereo(batch2.g[:2])
    ctx.synchronize()
    batch2.check_stereo(s1, (gl, "before"))
    batch2.check_track(t, gl)
    batch2.check_stereo(s2, (gl, "after"))


def test_keyframe_overlap_on_and_off(ctx, batch2, knobs):
    """the split stereo call followed by the keyframe detector, the chain beside the stereo kernels and behind them"""
    knobs(3, 1)
    cell, cap = 35, 2 * (W // 35) * (H // 35)
    cur = [k for k, _, _ in batch2.per]
    d_cur = ctx.to_device(np.concatenate(cur).astype(np.float32))
    d_cur_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(cur)]))
    n_cur = sum(len(c) for c in cur)
    res = []
    for on in (False, True):
        d_th = ctx.to_device(np.full(2, 0.001, np.float64))
        d_nout, d_out = ctx.to_device(np.full(2, -7, np.int32)), ctx.to_device(np.zeros((2, cap, 2), np.float32))
        call = batch2.stereo_call(ctx)
        ctx.set_kf_overlap(on)
        try:
            call.stereo(batch2.g[:2])
            fe.detect_grid_batch_dev(ctx, batch2.g[0], cell, 1, d_th, n_cur, d_cur, d_cur_img, None, d_nout, d_out, cap)
            ctx.synchronize()
        finally:
            ctx.set_kf_overlap(True)
        batch2.check_stereo(call, on)
        res.append([a.view(np.uint8) for a in call.get()] + [a.get().view(np.uint8) for a in (d_nout, d_out, d_th)])
    assert (res[0][3].view(np.int32) > 0).all()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
