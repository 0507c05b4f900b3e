"""The staged search region of the three-lane KLT kernels (ov2slam_amd/csrc/klt.hip, lk_level3): a level pass stages 14
rows x 32 bytes of the search image around its first window in LDS, the later iterations of the pass read their windows
from there, and an iteration whose window has left the region's row span (4 rows) or column span (20 bytes) fetches a new
region around it.  A narrow region can go wrong where a window crosses a span between two iterations of one pass and
where the region's origin is clamped at an image border, so every case here is chosen on the CPU to do one of the two:

  * the oracle's position after every iteration of every forward pass (one pass at a time on the level's own image, which
    reproduces the whole descent bit for bit -- asserted) goes through a model of the region: origin, spans and clamps as
    the kernel forms them.  A case asserts that its keypoints do re-stage (or do hit the clamp) before anything runs on
    the device, so it cannot pass without exercising the path;
  * the oracle itself tracks at least a few keypoints of every case.

Bar, as everywhere in the front end: status identical, positions bit-identical (float32 bit patterns), work words equal
to the oracle's LK iteration counts."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu

WIN, NLVL, PAD, LM = 9, 3, 9, 16
HALF = np.float32((WIN - 1) * 0.5)
# the region as klt3 lays it out
RROWS, RBYTES, ROW_MARGIN, ROW_SPAN, COL_LEAD, COL_ALIGN, COL_SPAN = 14, 32, 2, 4, 9, 4, 20
SIZES = (1, 20, 21, 22, 43)   # one keypoint, a wave less one, a full wave, a wave and one, two waves and one


def _istride(w):
    return (LM + w + PAD + 63) // 64 * 64


def _origin(inx, iny, w, h):
    """(rr0, cc0, clamps hit) of the region staged for a window whose first pixel is (inx, iny)"""
    r, c = iny + PAD - ROW_MARGIN, (LM + inx - COL_LEAD) & ~(COL_ALIGN - 1)
    rr0, cc0 = min(max(r, 0), h + 2 * PAD - RROWS), min(max(c, 0), _istride(w) - RBYTES)
    hit = set()
    if r < 0: hit.add("top")
    if r > h + 2 * PAD - RROWS: hit.add("bottom")
    if c < 0: hit.add("left")
    if c > _istride(w) - RBYTES: hit.add("right")
    return rr0, cc0, hit


def _inside(inx, iny, w, h):
    return not (inx < -WIN or inx >= w or iny < -WIN or iny >= h)


def _possible_clamps(w, h):
    """the clamps any window a pass may run on can hit on a w x h level"""
    hit = set()
    for iny in range(-WIN, h):
        for inx in range(-WIN, w):
            hit |= _origin(inx, iny, w, h)[2]
    return hit


def _region_events(traj, w, h):
    """what the region does during one pass whose iterations start from the positions `traj`: ({'row', 'col'} re-stages,
    clamps hit by any origin it forms)"""
    kinds, clamps = set(), set()
    win = [(int(np.floor(p[0] - HALF)), int(np.floor(p[1] - HALF))) for p in traj]
    in0 = _inside(*win[0], w, h)
    rr0, cc0, hit = _origin(win[0][0] if in0 else 0, win[0][1] if in0 else 0, w, h)
    if in0:
        clamps |= hit
    for inx, iny in win:
        if not _inside(inx, iny, w, h):
            break
        rb, cb = iny + PAD - rr0, LM + inx - cc0
        row, col = not 0 <= rb <= ROW_SPAN, not 0 <= cb <= COL_SPAN
        if row or col:
            kinds |= ({"row"} if row else set()) | ({"col"} if col else set())
            rr0, cc0, hit = _origin(inx, iny, w, h)
            clamps |= hit
    return kinds, clamps


class Scene:
    """an image pair, device and oracle pyramids, and the oracle's pyramids of every level's own image"""

    def __init__(self, ctx, oracle, I0, I1):
        self.oracle, self.h, self.w = oracle, *I0.shape
        self.raw = I0, I1
        self.g = fe.preprocess_image(ctx, I0, use_clahe=False), fe.preprocess_image(ctx, I1, use_clahe=False)
        self.o = oracle.Pyramid(I0), oracle.Pyramid(I1)
        self.lv = [self._levels(p) for p in self.o]
        self.dims = [self.o[0].level(l)[2:4] for l in range(self.o[0].nlevels)]

    def top(self, nl):
        """the level a descent of `nl` levels starts on: the pyramid ends where a level would not be larger than the window"""
        return min(nl, len(self.dims) - 1)

    def _levels(self, P):
        out = []
        for l in range(P.nlevels):
            img, _, w, h, pad = P.level(l)
            out.append(self.oracle.Pyramid(np.ascontiguousarray(img[pad:pad + h, pad:pad + w]), WIN, 0))
        return out

    def descent(self, kp, start, nl):
        """the forward passes of one keypoint, level nl .. 0: ({level: positions the pass's iterations start from},
        final position, status); max_iter = k stops a pass after k iterations, so its result is where iteration k starts"""
        lk = self.oracle.calc_optical_flow_pyr_lk
        kp, pos, traj, st = np.float32(kp).reshape(1, 2), np.float32(start).reshape(1, 2), {}, 0
        for l in range(self.top(nl), -1, -1):
            sc = np.float32(2.0 ** -l)
            s = pos * sc if l == self.top(nl) else pos * np.float32(2)
            fin, st, _, it = lk(self.lv[0][l], self.lv[1][l], kp * sc, s, WIN, 0, 30, 0.01)
            traj[l] = [s[0]] + [lk(self.lv[0][l], self.lv[1][l], kp * sc, s, WIN, 0, k, 0.01)[0][0] for k in range(1, int(it[0, 0]))]
            pos = fin
        return traj, pos[0], int(st[0])

    def events(self, kps, starts, nl):
        """per keypoint: {(level, 'row' / 'col')} re-stages and {(level, clamp)} of its forward passes; the pass-by-pass
        descent is the oracle's own (bit for bit)"""
        ref = self.oracle.calc_optical_flow_pyr_lk(*self.o, kps, starts, WIN, nl, 30, 0.01)[0]
        out = []
        for i in range(len(kps)):
            traj, pos, _ = self.descent(kps[i], starts[i], nl)
            assert np.array_equal(pos.view(np.uint32), ref[i].view(np.uint32))
            ev = [(l,) + _region_events(t, *self.dims[l]) for l, t in traj.items()]
            out.append(({(l, k) for l, ks, _ in ev for k in ks}, {(l, c) for l, _, cs in ev for c in cs}))
        return out


def _views(w, h, seed, *shifts):
    """[I0, I1, ...]: I_k shows I0's content moved by (-dx_k, -dy_k)"""
    m = 16
    tex = synth.base_texture(h + 2 * m, w + 2 * m, seed=seed)
    return [np.ascontiguousarray(tex[m + dy:m + dy + h, m + dx:m + dx + w]).astype(np.uint8) for dx, dy in ((0, 0),) + shifts]


@pytest.fixture(scope="module")
def three_lanes(ctx):
    ctx.set_klt_lanes(3)
    try:
        yield ctx
    finally:
        ctx.set_klt_lanes(0)


def _oracle_each(oracle, o0, o1, kps, pri, nl):
    out, st, it = np.empty_like(kps), np.zeros(len(kps), bool), np.zeros(len(kps), np.int64)
    for i in range(len(kps)):
        o, s, t = oracle.fb_klt_tracking(o0, o1, kps[i:i + 1], pri[i:i + 1], WIN, nl, 30.0, 0.5, 30, 0.01)
        out[i], st[i], it[i] = o[0], bool(s[0]), t
    return out, st, it


def _track_dev(ctx, g, kps, pri, nl):
    """ov2_klt_track_fb_dev: (positions, status, work words = iterations | level passes << 16)"""
    n = len(kps)
    d_k, d_p = ctx.to_device(kps), ctx.to_device(pri)
    d_s, d_w = ctx.to_device(np.full(n, 9, np.uint8)), ctx.to_device(np.full(n, 0xdeadbeef, np.uint32))
    fe.FeatureTracker(ctx, 30, 0.01).fbKltTracking_dev(g[0], g[1], WIN, nl, 30.0, 0.5, d_k, d_p, d_s, n, None, d_w)
    ctx.synchronize()
    return d_p.get(), d_s.get(), d_w.get()


def _assert_same(got, want, what):
    out, st, work = got
    eout, est, eit = want
    assert set(np.unique(st)) <= {0, 1}, what
    assert np.array_equal(st.astype(bool), est), what
    assert np.array_equal(out.view(np.uint32), eout.view(np.uint32)), what
    assert np.array_equal((work & 0xffff).astype(np.int64), eit), what
    assert (work >> 16).max() <= NLVL + 2, what


# ---- a window that leaves the region between two iterations of one pass ---------------------------------------------

SHIFT = (2, 1)                                      # content moves by (-2, -1) between the two images
OFFSETS = {"x": [(11, 0), (-12, 0), (13, 0)], "y": [(0, 5), (0, -5), (0, 4)], "xy": [(11, 4), (-11, -5), (12, -4)]}
NEED = {"x": {"col"}, "y": {"row"}, "xy": {"row", "col"}}


@pytest.fixture(scope="module")
def scene(three_lanes, oracle):
    return Scene(three_lanes, oracle, *_views(233, 121, 5, SHIFT))


@pytest.fixture(scope="module")
def crossing(scene, oracle):
    """per kind of offset and pyramid depth nl (0: the offset is crossed on level 0, 1: twice the offset, crossed on level
    1): 43 keypoints whose prior is that far off, the ones that re-stage as NEED says AND track in the oracle in front"""
    rng = np.random.default_rng(2)
    kps = np.stack([rng.uniform(30, scene.w - 30, 900), rng.uniform(24, scene.h - 24, 900)], 1).astype(np.float32)
    out = {}
    for kind, offs in OFFSETS.items():
        for nl in (0, 1):
            off = np.float32([offs[i % len(offs)] for i in range(len(kps))]) * np.float32(1 << nl)
            pri = kps - np.float32(SHIFT) + off
            want = _oracle_each(oracle, *scene.o, kps, pri, nl)
            ev = scene.events(kps, pri, nl)
            hit = np.array([NEED[kind] <= {k for l, k in e[0] if l == nl} for e in ev])   # on the starting level
            order = np.argsort(~(hit & want[1]), kind="stable")[:max(SIZES)]
            assert (hit & want[1])[order].sum() >= 3, (kind, nl, int(hit.sum()), int(want[1].sum()))
            assert hit[order[0]] and want[1][order[0]]
            out[kind, nl] = (kps[order], pri[order]) + tuple(a[order] for a in want)
    return out


@pytest.mark.parametrize("nl", [0, 1])
@pytest.mark.parametrize("kind", ["x", "y", "xy"])
def test_window_leaves_the_region_mid_pass(three_lanes, scene, crossing, kind, nl):
    """priors several pixels off in x, in y and in both: the pass walks out of the staged region's column span, row span
    or both and re-stages between two of its iterations; every call size around the wave, the re-staging keypoint first
    (n = 1 is that keypoint alone in its wave)"""
    kps, pri, *want = crossing[kind, nl]
    for n in SIZES:
        _assert_same(_track_dev(three_lanes, scene.g, kps[:n], pri[:n], nl), tuple(a[:n] for a in want), (kind, nl, n))


# ---- region origins clamped at the image borders ---------------------------------------------------------------------

SMALL = {"96x64": (96, 64), "96x80": (96, 80)}


@pytest.fixture(scope="module")
def small(three_lanes, oracle):
    return {k: Scene(three_lanes, oracle, *_views(w, h, 9, SHIFT)) for k, (w, h) in SMALL.items()}


def _border_case(sc, nl):
    """(keypoints in a band along and just outside every border of the starting level plus some inside, priors, clamps
    their first passes hit on the starting level)"""
    w, h, t = sc.w, sc.h, sc.top(nl)
    rng = np.random.default_rng(3 + nl)
    band = lambda lo, hi, n: rng.uniform(lo, hi, n)
    lo, hi = -5 << t, 3 << t
    edge = np.concatenate([np.stack([band(lo, hi, 16), band(0, h, 16)], 1), np.stack([band(w - hi, w - lo, 16), band(0, h, 16)], 1),
                           np.stack([band(0, w, 16), band(lo, hi, 16)], 1), np.stack([band(0, w, 16), band(h - hi, h - lo, 16)], 1)])
    inner = np.stack([band(14, w - 14, 16), band(14, h - 14, 16)], 1)
    kps = np.concatenate([edge, inner]).astype(np.float32)
    kps = kps[rng.permutation(len(kps))]
    pri = kps - np.float32(SHIFT) + rng.normal(0, 0.7, kps.shape).astype(np.float32)
    hit = {c for e in sc.events(kps, pri, nl) for l, c in e[1] if l == t}
    return kps, pri, hit


@pytest.mark.parametrize("nl", [0, 3])
@pytest.mark.parametrize("size", list(SMALL))
def test_region_origin_clamped_at_every_border(three_lanes, oracle, small, size, nl):
    """keypoints in a band along and just outside every border, tracked on level 0 alone and on the whole pyramid, whose top
    level is a window or two wide.  96 x 64 has no level 3 (12 x 8 is no larger than the 9 x 9 window, where
    buildOpticalFlowPyramid ends the pyramid: both sides start a descent of three levels on level 2, 24 x 16); 96 x 80 has
    one (12 x 10).  Every clamp of the origin that the starting level's geometry allows -- rows at 0 and at rows - 14,
    columns at 0 and at the row pitch - 32 -- is hit there, and the keypoints inside track"""
    sc = small[size]
    assert sc.top(3) == (2 if size == "96x64" else 3)
    kps, pri, hit = _border_case(sc, nl)
    assert hit == _possible_clamps(*sc.dims[sc.top(nl)]) and {"top", "bottom", "left"} <= hit, (size, nl, hit)
    assert nl != 0 or "right" in hit
    want = _oracle_each(oracle, *sc.o, kps, pri, nl)
    assert want[1].sum() >= 8
    _assert_same(_track_dev(three_lanes, sc.g, kps, pri, nl), want, (size, nl))


# ---- one kltTracking call and one stereoMatching call on a batch of two, split descent on and off ---------------------

class Batch2:
    """two image triples (previous, current = moved by SHIFT, right = moved by (6, 0)) as batched pyramids, keypoints of
    both images interleaved.  A third of the keypoints has no prior; the priors of the others are off by the crossing
    offsets (twice the level-0 offsets: list A crosses them on level 1), a few by 0.5 px"""

    def __init__(self, ctx, oracle):
        w, h, self.n_img = 233, 121, 60
        trip = []
        for b in range(2):
            trip.append(_views(w, h, 21 + b, SHIFT, (6, 0)))
        self.keep = []
        self.g = [self._pyr(ctx, [t[k] for t in trip], w, h) for k in range(3)]
        self.sc = [[Scene(ctx, oracle, t[0], t[k]) for k in (1, 2)] for t in trip]     # [image][current / right]
        rng = np.random.default_rng(6)
        self.per = []
        for b in range(2):
            kps = np.stack([rng.uniform(30, w - 30, self.n_img), rng.uniform(24, h - 24, self.n_img)], 1).astype(np.float32)
            offs = [o for k in ("x", "y", "xy") for o in OFFSETS[k]] + [(0.5, 0.0)]
            off = np.float32([offs[i % len(offs)] for i in range(self.n_img)]) * np.float32(2)
            has = (np.arange(self.n_img) % 3 != 0).astype(np.uint8)
            self.per.append((kps, off, has))
        self.perm = np.random.default_rng(8).permutation(2 * self.n_img)
        self.idx = np.repeat(np.arange(2, dtype=np.int32), self.n_img)[self.perm]

    def _pyr(self, ctx, imgs, w, h):
        im = fe.Images(ctx, 2, w, h)
        for b, I in enumerate(imgs):
            im.upload(b, I)
        self.keep.append(im)
        return fe.preprocess_images(ctx, im, use_clahe=False)

    def inputs(self, shift, far_b):
        """(kps, prior, has_prior) per image for content moved by `shift`; a keypoint without a prior carries its own
        position (kltTracking ignores it) or, `far_b`, a start 28 - 30 px off in y for stereoMatching's full pyramid: 3.5 px
        on level 3, which leaves the row span there"""
        out = []
        for kps, off, has in self.per:
            far = np.float32([(0, 28), (0, -30), (3, 29)])[np.arange(len(kps)) % 3] if far_b else np.float32(0)
            own = kps - np.float32(shift) + far if far_b else kps
            pri = np.where(has[:, None] != 0, kps - np.float32(shift) + off, own).astype(np.float32)
            out.append((kps, pri, has))
        return out

    def flat(self, per):
        return tuple(np.ascontiguousarray(np.concatenate([p[k] for p in per])[self.perm]) for k in range(3))

    def rows(self, b):
        r = np.flatnonzero(self.idx == b)
        return r[np.argsort(self.perm[r])]

    def restaged(self, k, per, own):
        """the kinds of re-stage the first pass over each list performs somewhere in the batch: list A on two levels from the
        prior, the no-prior list on the full pyramid from `own` position or from the prior"""
        kinds = {"A": set(), "B": set()}
        for b, (kps, pri, has) in enumerate(per):
            a, nb = has != 0, has == 0
            for e in self.sc[b][k].events(kps[a], pri[a], 1):
                kinds["A"] |= {kd for _, kd in e[0]}
            for e in self.sc[b][k].events(kps[nb], kps[nb] if own else pri[nb], NLVL):
                kinds["B"] |= {kd for _, kd in e[0]}
        return kinds


@pytest.fixture(scope="module")
def batch2(three_lanes, oracle):
    return Batch2(three_lanes, oracle)


def _two_stage(ctx, which, g0, g1, kps, pri, has, idx):
    n = len(kps)
    trk = fe.FeatureTracker(ctx, 30, 0.01)
    d_in = [ctx.to_device(a) for a in (kps, pri, has)]
    d_o, d_s = ctx.to_device(np.full((n, 2), -777.0, np.float32)), ctx.to_device(np.full(n, 9, np.uint8))
    d_w, d_i = ctx.to_device(np.full(2 * n, 0xdeadbeef, np.uint32)), ctx.to_device(idx)
    if which == "track":
        d_r = ctx.to_device(np.full(2, -1, np.int32))
        trk.kltTracking_dev(g0, g1, WIN, NLVL, 30.0, 0.5, *d_in, d_o, d_s, n, d_i, d_r, d_w)
    else:
        d_r = None
        trk.stereoMatching_dev(g0, g1, WIN, NLVL, 30.0, 0.5, *d_in, d_o, d_s, n, d_i, None, True, None, d_iters=d_w)
    ctx.synchronize()
    return d_o.get(), d_s.get(), d_w.get(), None if d_r is None else d_r.get()


def _list_words(oracle, o0, o1, kps, pri, has, own, drop):
    """LK iterations the work words must show: the two-level pass of a keypoint with a prior in word i, the full-pyramid pass
    (no prior: from its own position or from `pri`; a failure of the two-level pass: from the failed forward result, or
    from the keypoint when the image dropped its priors) in word n + i"""
    a = has != 0
    it_a, it_f = np.zeros(len(kps), np.int64), np.zeros(len(kps), np.int64)
    fwd, st, it_a[a] = _oracle_each(oracle, o0, o1, kps[a], pri[a], 1)
    fail = np.flatnonzero(a)[~st]
    it_f[fail] = _oracle_each(oracle, o0, o1, kps[fail], kps[fail] if drop else fwd[~st], NLVL)[2]
    it_f[~a] = _oracle_each(oracle, o0, o1, kps[~a], kps[~a] if own else pri[~a], NLVL)[2]
    return it_a, it_f, len(fail)


@pytest.mark.parametrize("split", ["on", "off"])
def test_tracking_and_stereo_calls_on_a_batch_of_two(three_lanes, oracle, batch2, split):
    """ov2_klt_tracking_frame_dev and ov2_stereo_matching_dev on two images with interleaved image indices, stereoMatching's
    no-prior descent split across the two launches (resumed on level 1) and whole in the second launch: per image
    positions, status and work words against the oracle.  The priors cross the region's spans on level 1 of list A, the
    failures go on to the re-tracking list, and stereoMatching's no-prior list leaves the row span on level 3 -- with the
    split that is the first launch's upper form"""
    ctx = three_lanes
    for which, k, shift in (("track", 0, SHIFT), ("stereo", 1, (6, 0))):
        per = batch2.inputs(shift, far_b=which == "stereo")
        kinds = batch2.restaged(k, per, own=which == "track")
        assert {"row", "col"} <= kinds["A"] and (which == "track" or "row" in kinds["B"]), (which, kinds)
        kps, pri, has = batch2.flat(per)
        ctx.set_stereo_split(1 if split == "on" else NLVL + 1)
        try:
            out, st, work, p3p = _two_stage(ctx, which, batch2.g[0], batch2.g[1 + k], kps, pri, has, batch2.idx)
        finally:
            ctx.set_stereo_split(-1)
        n = len(kps)
        for b in range(2):
            r = batch2.rows(b)
            o0, o1 = batch2.sc[b][k].o
            if which == "track":
                eo, es, ep = oracle.klt_tracking_frame(o0, o1, *per[b])
                assert bool(p3p[b]) == ep, (which, split, b)
            else:
                eo, es = oracle.stereo_matching(o0, o1, *per[b])
                ep = False
            assert np.array_equal(st[r].astype(bool), es.astype(bool)), (which, split, b)
            assert np.array_equal(out[r].view(np.uint32), eo.view(np.uint32)), (which, split, b)
            it_a, it_f, n_fail = _list_words(oracle, o0, o1, *per[b], own=which == "track", drop=ep)
            assert np.array_equal((work[r] & 0xffff).astype(np.int64), it_a), (which, split, b)
            assert np.array_equal((work[n + r] & 0xffff).astype(np.int64), it_f), (which, split, b)
            assert n_fail >= 2 and es.astype(bool).sum() >= 8, (which, split, b, n_fail, int(es.sum()))
