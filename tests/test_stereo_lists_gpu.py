"""Which launch tracks which list (ov2slam_amd/csrc/klt.hip, ov2_klt_two_stage_dev): for stereoMatching the first launch
tracks list A (keypoints with a prior, two levels) alone and the second launch tracks list B (no prior, full pyramid) in a
leading segment of workgroups in front of list C (the failures of A, re-tracked on the full pyramid); for kltTracking list
B stays in the first launch and the second launch's B segment is empty.  Every case compares positions (float32 bit
patterns) and status with the oracle's stereo_matching / klt_tracking_frame, and the work words with the layout the C ABI
documents: list-A passes in iters[i], full-pyramid passes in iters[n + i] (low 16 bits = LK iterations).

The list lengths are chosen around the keypoints per wave of each mapping (21, 8, 4): a segment that is empty, one
keypoint, one short of a wave, a full wave, one more, two waves and one.  List C is forced with priors 6-10 px off, and
the oracle (two levels, one keypoint at a time) says which of them really fail before a case uses them."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu

W, H = 752, 480
WIN, NLVL = 9, 3
KPW = {3: 21, 8: 8, 16: 4}                 # lanes per keypoint -> keypoints per wave
N_EASY = 30                                # list-A keypoints that track, in every list-length case
MAX_B, MAX_C = 2 * 21 + 1, 21 + 1


def _lengths(k):
    return [(nb, nc) for nb in (0, 1, k - 1, k, k + 1, 2 * k + 1) for nc in (0, 1, k, k + 1)]


def _each(oracle, o0, o1, kps, pri, nl):
    """the oracle one keypoint at a time: (forward result, status, LK iterations) of each"""
    out, st, it = np.empty_like(kps), np.zeros(len(kps), bool), np.zeros(len(kps), np.int64)
    for i in range(len(kps)):
        o, s, t = oracle.fb_klt_tracking(o0, o1, kps[i:i + 1], pri[i:i + 1], WIN, nl, 30.0, 0.5, 30, 0.01)
        out[i], st[i], it[i] = o[0], bool(s[0]), t
    return out, st, it


def _words(oracle, o0, o1, kps, pri, has, own=False, drop=False):
    """what the work words of one image's keypoints must say, from the oracle one keypoint at a time: (has_prior, LK
    iterations of the two-level pass, of the full-pyramid pass, who takes the full-pyramid pass).  Keypoints with a prior
    take the two-level pass, and its failures the full pyramid from the failed forward result (kltTracking with under 33 %
    tracked, `drop`: from the keypoint itself); keypoints without one take the full pyramid from `pri` (stereoMatching) or
    from their own position (kltTracking, `own`)"""
    has = np.asarray(has) != 0
    it_a, it_full = np.zeros(len(kps), np.int64), np.zeros(len(kps), np.int64)
    fwd, st, it_a[has] = _each(oracle, o0, o1, kps[has], pri[has], 1)
    fail = np.flatnonzero(has)[~st]
    it_full[fail] = _each(oracle, o0, o1, kps[fail], kps[fail] if drop else fwd[~st], NLVL)[2]
    it_full[~has] = _each(oracle, o0, o1, kps[~has], kps[~has] if own else pri[~has], NLVL)[2]
    full = ~has
    full[fail] = True
    return has, it_a, it_full, full


def _check_words(w_a, w_full, has, it_a, it_full, full, what):
    """the layout of the work words: the two-level pass of a keypoint with a prior in iters[i], the full-pyramid pass (no
    prior, or a failure re-tracked) in iters[n + i], low 16 bits = LK iterations; a keypoint that takes no part in a
    stage has a zero word there"""
    assert np.array_equal((w_a & 0xffff).astype(np.int64), it_a), what
    assert np.array_equal((w_full & 0xffff).astype(np.int64), it_full), what
    assert np.array_equal(w_a == 0, np.asarray(has) == 0), what
    assert np.array_equal(w_full == 0, ~full), what
    assert max((w_a >> 16).max(), (w_full >> 16).max()) <= NLVL + 2, what


class Pools:
    """one 752 x 480 stereo pair, device and oracle pyramids, and three disjoint pools of keypoints with what the oracle
    says about each: `b` (no prior: full pyramid from the keypoint's own left position), `c` (prior 6-10 px off that
    FAILS on two levels, then the full pyramid from the failed forward result) and `a` (prior that tracks on two levels)"""

    def __init__(self, ctx, oracle, stream, t):
        L, R = stream.left(t), stream.right(t)
        self.g = fe.preprocess_image(ctx, L, use_clahe=False), fe.preprocess_image(ctx, R, use_clahe=False)
        self.o = oracle.Pyramid(L), oracle.Pyramid(R)
        self.raw = L, R
        rng = np.random.default_rng(100 + t)
        kps = synth.grid_keypoints(360, seed=40 + t)
        kps = kps[rng.permutation(len(kps))]
        gt = stream.stereo_gt(kps).astype(np.float32)
        kb, kc, ka = kps[:MAX_B], kps[MAX_B:MAX_B + 200], kps[MAX_B + 200:MAX_B + 200 + 2 * N_EASY]
        # list B
        _, _, it = _each(oracle, *self.o, kb, kb, NLVL)
        self.b = dict(kps=kb, pri=kb.copy(), it_a=np.zeros(len(kb), np.int64), it_full=it, full=np.ones(len(kb), bool))
        # list C: off by 6-10 px in a random direction, kept where the two-level pass fails
        ang, r = rng.uniform(0, 2 * np.pi, len(kc)), rng.uniform(6.0, 10.0, len(kc))
        pc = (gt[MAX_B:MAX_B + 200] + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)).astype(np.float32)
        fwd, st, it = _each(oracle, *self.o, kc, pc, 1)
        fail = np.flatnonzero(~st)[:MAX_C]
        assert len(fail) == MAX_C, f"only {len(fail)} of {len(kc)} far priors fail on two levels"
        _, _, it2 = _each(oracle, *self.o, kc[fail], fwd[fail], NLVL)
        self.c = dict(kps=kc[fail], pri=pc[fail], it_a=it[fail], it_full=it2, full=np.ones(MAX_C, bool))
        # list A that tracks
        pa = (gt[MAX_B + 200:MAX_B + 200 + 2 * N_EASY] + rng.normal(0, 0.5, ka.shape)).astype(np.float32)
        _, st, it = _each(oracle, *self.o, ka, pa, 1)
        good = np.flatnonzero(st)[:N_EASY]
        assert len(good) == N_EASY
        self.a = dict(kps=ka[good], pri=pa[good], it_a=it[good], it_full=np.zeros(N_EASY, np.int64), full=np.zeros(N_EASY, bool))
        self.cases = {}

    def case(self, oracle, nb, nc, na, seed=0):
        """(kps, prior, has_prior, expected positions, status, iterations of the two-level pass, of the full-pyramid pass,
        who takes the full-pyramid pass) of nb / nc / na keypoints of the three pools in a random order; the oracle runs
        once per shape"""
        key = (nb, nc, na, seed)
        if key not in self.cases:
            parts = [(self.b, nb, 0), (self.c, nc, 1), (self.a, na, 1)]
            cat = lambda f: np.concatenate([p[f][:k] for p, k, _ in parts])
            has = np.concatenate([np.full(k, h, np.uint8) for _, k, h in parts])
            perm = np.random.default_rng(7 + seed + 100 * nb + nc).permutation(len(has))
            kps, pri, has, it_a, it_full, full = (np.ascontiguousarray(a[perm]) for a in
                                                  (cat("kps"), cat("pri"), has, cat("it_a"), cat("it_full"), cat("full")))
            # the case has the intended lists: |C| = list-A keypoints that fail on two levels
            if has.any():
                _, st1, _ = oracle.fb_klt_tracking(*self.o, kps[has != 0], pri[has != 0], WIN, 1, 30.0, 0.5, 30, 0.01)
                assert int((st1 == 0).sum()) == nc
            else:
                assert nc == 0
            assert int((has == 0).sum()) == nb
            exy, est = oracle.stereo_matching(*self.o, kps, pri, has)
            self.cases[key] = (kps, pri, has, exy, est, it_a, it_full, full)
        return self.cases[key]


@pytest.fixture(scope="module")
def pools(ctx, oracle, stream):
    return Pools(ctx, oracle, stream, 0)


@pytest.fixture
def lanes(ctx):
    def choose(n):
        ctx.set_klt_lanes(n)
    try:
        yield choose
    finally:
        ctx.set_klt_lanes(0)


class Call:
    """the device-resident arguments and outputs of one tracking call, uploaded before anything is enqueued and held until
    the results are read: an upload waits for the stream and a freed array for the whole device, so a call that made them
    on its way would never be in flight together with the call after it.  Every output starts from a pattern the call
    must overwrite"""

    def __init__(self, ctx, kps, pri, has, img_idx=None, batch=0):
        n = self.n = len(kps)
        self.trk = fe.FeatureTracker(ctx, 30, 0.01)
        self.d_in = [ctx.to_device(np.ascontiguousarray(a, t)) for a, t in ((kps, np.float32), (pri, np.float32), (has, np.uint8))]
        self.d_i = None if img_idx is None else ctx.to_device(np.ascontiguousarray(img_idx, np.int32))
        self.d_o = ctx.to_device(np.full((n, 2), -777.0, np.float32))
        self.d_s = ctx.to_device(np.full(n, 9, np.uint8))
        self.d_w = ctx.to_device(np.full(2 * n, 0xdeadbeef, np.uint32))
        self.d_r = ctx.to_device(np.full(batch, -1, np.int32)) if batch else None

    def stereo(self, g):
        """ov2_stereo_matching_dev, enqueued"""
        self.trk.stereoMatching_dev(g[0], g[1], WIN, NLVL, 30.0, 0.5, *self.d_in, self.d_o, self.d_s, self.n, self.d_i, None,
                                    True, None, d_iters=self.d_w)
        return self

    def track(self, g):
        """ov2_klt_tracking_frame_dev, enqueued"""
        self.trk.kltTracking_dev(g[0], g[1], WIN, NLVL, 30.0, 0.5, *self.d_in, self.d_o, self.d_s, self.n, self.d_i, self.d_r,
                                 self.d_w)
        return self

    def get(self):
        """(positions, status, work words [2n]) once the caller has synchronised"""
        return self.d_o.get(), self.d_s.get(), self.d_w.get()


def _check_stereo(call, case, what):
    kps, pri, has, exy, est, it_a, it_full, full = case
    n = len(kps)
    out, st, work = call.get()
    assert np.array_equal(st.astype(bool), est), what
    assert set(np.unique(st)) <= {0, 1}, what
    assert np.array_equal(out.view(np.uint32), exy.view(np.uint32)), what
    _check_words(work[:n], work[n:], has, it_a, it_full, full, what)


@pytest.mark.parametrize("gl,nb,nc", [(gl, nb, nc) for gl in (3, 8, 16) for nb, nc in _lengths(KPW[gl])])
def test_list_lengths_around_the_wave(ctx, oracle, pools, lanes, gl, nb, nc):
    lanes(gl)
    case = pools.case(oracle, nb, nc, N_EASY)
    got = Call(ctx, *case[:3]).stereo(pools.g)
    ctx.synchronize()
    _check_stereo(got, case, (gl, nb, nc))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_single_list_calls(ctx, oracle, pools, lanes, gl):
    """no keypoint has a prior (list A and list C empty: the first launch has nothing to do), and every keypoint has one
    (list B empty in both launches), with and without failures to re-track"""
    lanes(gl)
    k = KPW[gl]
    for nb, nc, na in ((2 * k + 1, 0, 0), (0, 0, N_EASY), (0, k + 1, N_EASY), (0, k + 1, 0)):
        case = pools.case(oracle, nb, nc, na)
        got = Call(ctx, *case[:3]).stereo(pools.g)
        ctx.synchronize()
        _check_stereo(got, case, (gl, nb, nc, na))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_one_keypoint(ctx, oracle, pools, lanes, gl):
    lanes(gl)
    for nb, nc, na in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        case = pools.case(oracle, nb, nc, na)
        assert len(case[0]) == 1
        got = Call(ctx, *case[:3]).stereo(pools.g)
        ctx.synchronize()
        _check_stereo(got, case, (gl, nb, nc, na))


class Batch2:
    """two stereo pairs and the frame that follows each as batched pyramids; image 0 carries a case of the pools, image 1
    the usual mix (70 % priors 1 px off) with a few priors 8 px off; keypoints interleaved by a permutation"""

    def __init__(self, ctx, oracle, stream, pools):
        L = [pools.raw[0], stream.left(3)]
        R = [pools.raw[1], stream.right(3)]
        N = [stream.left(3), stream.left(6)]
        self.keep = []
        self.g = [self._pyr(ctx, I) for I in (L, R, N)]
        self.o = [[oracle.Pyramid(i) for i in I] for I in (L, R, N)]
        k0, p0, h0 = pools.case(oracle, 9, 5, N_EASY, seed=1)[:3]
        k1 = synth.grid_keypoints(70, seed=61)
        p1, h1 = synth.make_priors(k1, stream.stereo_gt(k1), seed=62)
        p1[np.flatnonzero(h1)[:6]] += np.float32(8.0)
        self.per = [(k0, p0, h0), (k1, p1, h1)]
        n0, n1 = len(k0), len(k1)
        self.perm = np.random.default_rng(5).permutation(n0 + n1)
        self.idx = np.concatenate([np.zeros(n0, np.int32), np.ones(n1, np.int32)])[self.perm]
        self.kps, self.pri, self.has = (np.ascontiguousarray(np.concatenate([a, b])[self.perm]) for a, b in zip(*self.per))
        self.stereo = [oracle.stereo_matching(self.o[0][b], self.o[1][b], *self.per[b]) for b in range(2)]
        # kltTracking left(t) -> left(t + 3): image 0 with priors 1 px off and a few 8 px off, image 1 with priors 25 px off (under 33 % tracked)
        self.tpri = []
        for b, t in enumerate((0, 3)):
            kb = self.per[b][0]
            self.tpri.append(synth.make_priors(kb, stream.flow(t, t + 3, kb), sigma=25.0 if b else 1.0, seed=80 + b))
        self.tpri[0][0][np.flatnonzero(self.tpri[0][1])[:6]] += np.float32(8.0)   # failures to re-track where the priors are kept, too
        self.tp, self.th = (np.ascontiguousarray(np.concatenate([a, b])[self.perm]) for a, b in zip(*self.tpri))
        self.track = [oracle.klt_tracking_frame(self.o[0][b], self.o[2][b], self.per[b][0], *self.tpri[b]) for b in range(2)]
        assert [t[2] for t in self.track] == [False, True]   # both outcomes of the 33 % rule
        # the work words each call must leave, per image in the image's own keypoint order
        self.stereo_words = [_words(oracle, self.o[0][b], self.o[1][b], *self.per[b]) for b in range(2)]
        self.track_words = [_words(oracle, self.o[0][b], self.o[2][b], self.per[b][0], *self.tpri[b], own=True, drop=self.track[b][2])
                            for b in range(2)]
        for b in range(2):   # list C spans both images in the stereo call, and the tracking call re-tracks in both
            assert (self.stereo_words[b][3] & self.stereo_words[b][0]).any() and (self.track_words[b][3] & self.track_words[b][0]).any()

    def _pyr(self, ctx, imgs):
        im = fe.Images(ctx, 2, W, H)
        for b, I in enumerate(imgs):
            im.upload(b, I)
        self.keep.append(im)
        return fe.preprocess_images(ctx, im, use_clahe=False)

    def rows(self, b):
        r = np.flatnonzero(self.idx == b)
        return r[np.argsort(self.perm[r])]      # the image's own keypoint order

    def check_words(self, work, exp, what):
        n = len(self.kps)
        for b in range(2):
            r = self.rows(b)
            _check_words(work[r], work[n + r], *exp[b], (what, b))

    def check_stereo(self, call, what):
        out, st, work = call.get()
        for b in range(2):
            exy, est = self.stereo[b]
            assert np.array_equal(st[self.rows(b)].astype(bool), est), (what, b)
            assert np.array_equal(out[self.rows(b)].view(np.uint32), exy.view(np.uint32)), (what, b)
        self.check_words(work, self.stereo_words, what)

    def check_track(self, call, what):
        out, st, work = call.get()
        p3p = call.d_r.get()
        for b in range(2):
            eo, es, ep = self.track[b]
            assert bool(p3p[b]) == ep, (what, b)
            assert np.array_equal(st[self.rows(b)].astype(bool), es.astype(bool)), (what, b)
            assert np.array_equal(out[self.rows(b)].view(np.uint32), eo.view(np.uint32)), (what, b)
        self.check_words(work, self.track_words, what)

    def stereo_call(self, ctx):
        return Call(ctx, self.kps, self.pri, self.has, self.idx)

    def track_call(self, ctx):
        return Call(ctx, self.kps, self.tp, self.th, self.idx, batch=2)


@pytest.fixture(scope="module")
def batch2(ctx, oracle, stream, pools):
    return Batch2(ctx, oracle, stream, pools)


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_batch_of_two_interleaved(ctx, batch2, lanes, gl):
    lanes(gl)
    got = batch2.stereo_call(ctx).stereo(batch2.g[:2])
    ctx.synchronize()
    batch2.check_stereo(got, gl)


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_tracking_between_stereo_calls(ctx, batch2, lanes, gl):
    """stereo, kltTracking (33 % rule: image 0 keeps its re-queued priors, image 1 drops them and raises its flag), stereo:
    the arguments of all three are on the device first, then the three calls are enqueued with nothing synchronised in
    between, so the counter double buffer and the zero word serve calls in one stream that hand list B to different
    launches.  Positions, status and work words of each call against the oracle"""
    lanes(gl)
    s1, t, s2 = batch2.stereo_call(ctx), batch2.track_call(ctx), batch2.stereo_call(ctx)
    s1.stereo(batch2.g[:2])
    t.track((batch2.g[0], batch2.g[2]))
    s2.stereo(batch2.g[:2])
    ctx.synchronize()
    batch2.check_stereo(s1, (gl, "before"))
    batch2.check_track(t, gl)
    batch2.check_stereo(s2, (gl, "after"))


def test_keyframe_overlap_on_and_off(ctx, batch2):
    """the stereo call followed by the keyframe detector on the left pyramid, with the detector chain beside the stereo
    kernels (ov2_ctx_set_kf_overlap) and behind them: same statuses, positions, work words, corner counts and corners, and
    the stereo part equal to the oracle both ways.  Every argument of both calls is on the device before the first is
    enqueued and nothing synchronises between them, so with the overlap on the detector does run beside the tracking
    launches"""
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
