"""GPU parity tests of the three-lane KLT mapping with 21 keypoints per wave (ov2slam_amd/csrc/klt.hip, klt_map<3>): keypoint
g of a wave sits on lanes 3g .. 3g + 2, so the groups of slots 5 and 10 straddle a 16-lane DPP row and their three-lane
sums go through the whole-wave shifts.  Bar, as everywhere in the front end: status identical, positions bit-identical
(float32 bit patterns), LK iteration counts identical to the scalar oracle; a keypoint's result does not depend on the
call size, on its slot in the wave or on the other images of the batch."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe, synth

pytestmark = pytest.mark.gpu

KPW = 21                      # keypoints per wave of the three-lane kernels
STRADDLE = (5, 10)            # slots whose lanes (15-17, 30-32) lie in two DPP rows
CALL_SIZES = (1, 2, 20, 21, 22, 41, 42, 43, 63, 64, 300)


def _texture_pair(w, h, seed, dx=2, dy=1, flat=None):
    """(I0, I1): I1 shows I0's content moved by (-dx, -dy); `flat` = (y0, y1, x0, x1) becomes a textureless block in both"""
    tex = synth.base_texture(h + 40, w + 40, seed=seed)
    I0 = np.ascontiguousarray(tex[10:10 + h, 10:10 + w]).astype(np.uint8)
    I1 = np.ascontiguousarray(tex[10 + dy:10 + dy + h, 10 + dx:10 + dx + w]).astype(np.uint8)
    if flat is not None:
        y0, y1, x0, x1 = flat
        I0[y0:y1, x0:x1] = 128
        I1[y0:y1, x0:x1] = 128
    return I0, I1


def _oracle_each(oracle, o0, o1, kps, pri, nl):
    """the oracle one keypoint at a time: positions, status and the LK iterations (all levels + backward pass) of each"""
    out, st, it = np.empty_like(kps), np.zeros(len(kps), bool), np.zeros(len(kps), np.int64)
    for i in range(len(kps)):
        o, s, t = oracle.fb_klt_tracking(o0, o1, kps[i:i + 1], pri[i:i + 1], 9, nl, 30.0, 0.5, 30, 0.01)
        out[i], st[i], it[i] = o[0], bool(s[0]), t
    return out, st, it


def _track_dev(ctx, g0, g1, kps, pri, nl, img_idx=None):
    """ov2_klt_track_fb_dev: (positions, status, work words = iterations | level passes << 16)"""
    n = len(kps)
    d_k, d_p = ctx.to_device(kps), ctx.to_device(pri)
    d_s, d_w = ctx.empty((n,), np.uint8), ctx.to_device(np.full(n, 0xdeadbeef, np.uint32))
    d_i = None if img_idx is None else ctx.to_device(np.ascontiguousarray(img_idx, np.int32))
    fe.FeatureTracker(ctx, 30, 0.01).fbKltTracking_dev(g0, g1, 9, nl, 30.0, 0.5, d_k, d_p, d_s, n, d_i, d_w)
    ctx.synchronize()
    return d_p.get(), d_s.get().astype(bool), d_w.get()


def _assert_same(got, want, what):
    out, st, work = got
    eout, est, eit = want
    assert np.array_equal(st, est), what
    assert np.array_equal(out.view(np.uint32), eout.view(np.uint32)), what
    assert np.array_equal((work & 0xffff).astype(np.int64), eit), what


@pytest.fixture(scope="module")
def three_lanes(ctx):
    ctx.set_klt_lanes(3)
    try:
        yield ctx
    finally:
        ctx.set_klt_lanes(0)


def _small_case(ctx, oracle, stream, name):
    """image pair + 300 keypoints anywhere in and a little outside the image, priors 1.5 px off"""
    if name == "752x480":
        I0, I1 = stream.left(0), stream.left(3)
    else:
        w, h = (int(v) for v in name.split("x"))
        I0, I1 = _texture_pair(w, h, seed=w)
    h, w = I0.shape
    rng = np.random.default_rng(w + h)
    n = max(CALL_SIZES)
    kps = np.stack([rng.uniform(-6, w + 6, n), rng.uniform(-6, h + 6, n)], 1).astype(np.float32)
    pri = kps + rng.normal(0, 1.5, kps.shape).astype(np.float32)
    g0, g1 = fe.preprocess_image(ctx, I0, use_clahe=False), fe.preprocess_image(ctx, I1, use_clahe=False)
    return g0, g1, oracle.Pyramid(I0), oracle.Pyramid(I1), kps, pri


@pytest.mark.parametrize("name", ["101x67", "233x121", "752x480"])
def test_call_sizes_around_the_wave(three_lanes, oracle, stream, name):
    """ov2_klt_track_fb_dev with n = 1 .. 300 keypoints (one lane group, a full wave, one keypoint more, two and three
    waves and their neighbours): the first n keypoints of one list, so one oracle run serves every size; positions,
    status and iteration counts equal the oracle, and the whole work word (with the level passes) of a keypoint is the
    same at every call size"""
    ctx = three_lanes
    g0, g1, o0, o1, kps, pri = _small_case(ctx, oracle, stream, name)
    for nl in (1, 3):
        want = _oracle_each(oracle, o0, o1, kps, pri, nl)
        full = None
        for n in sorted(CALL_SIZES, reverse=True):
            got = _track_dev(ctx, g0, g1, kps[:n], pri[:n], nl)
            _assert_same(got, tuple(a[:n] for a in want), (name, nl, n))
            if full is None:
                full = got[2]
                assert (full >> 16).max() <= nl + 2   # one pass per level forward and one backward
            assert np.array_equal(got[2], full[:n]), (name, nl, n)
        assert want[1].mean() > 0.2   # the case does track


def _hard_case(oracle):
    """233 x 121 pair with a flat block; eight hard keypoints (window partly outside the image on each side, priors 3 px
    off, textureless patch) and easy ones"""
    w, h = 233, 121
    I0, I1 = _texture_pair(w, h, seed=5, flat=(40, 80, 100, 150))
    hard = np.array([[1.3, 60.2], [231.6, 50.7], [117.4, 0.8], [90.1, 119.9],       # left / right / top / bottom
                     [60.5, 30.5], [180.2, 95.3],                                  # prior 3 px off (below)
                     [125.0, 60.0], [118.7, 55.1]], np.float32)                    # inside the flat block
    hpri = hard - np.float32([2.0, 1.0])
    hpri[4] += np.float32([3.0, 0.0])
    hpri[5] += np.float32([-2.1, 2.1])
    rng = np.random.default_rng(11)
    easy = np.stack([rng.uniform(15, 95, 200), rng.uniform(15, 105, 200)], 1).astype(np.float32)
    easy = easy[~((easy[:, 0] > 88) & (easy[:, 1] > 28) & (easy[:, 1] < 92))]      # clear of the flat block
    epri = easy - np.float32([2.0, 1.0]) + rng.normal(0, 0.3, easy.shape).astype(np.float32)
    return I0, I1, hard, hpri, easy, epri


def _layout(hard_slots, n_hard, n_waves):
    """index lists: which keypoint (hard h >= 0 coded as -1 - h, easy e >= 0) sits at each position of n_waves full waves"""
    order, h, e = [], 0, 0
    for wv in range(n_waves):
        for s in range(KPW):
            if s in hard_slots and h < n_hard:
                order.append(-1 - h); h += 1
            else:
                order.append(e); e += 1
    assert h == n_hard
    return order


def test_straddling_groups(three_lanes, oracle):
    """the hardest keypoints in slots 5 and 10 of four waves with easy ones around them, then in the neighbouring slots 4 and
    11, then 6 and 9 (easy ones in 5 and 10): every layout equals the oracle and a keypoint's result -- work word
    included -- is the same wherever it sits"""
    ctx = three_lanes
    I0, I1, hard, hpri, easy, epri = _hard_case(oracle)
    g0, g1 = fe.preprocess_image(ctx, I0, use_clahe=False), fe.preprocess_image(ctx, I1, use_clahe=False)
    o0, o1 = oracle.Pyramid(I0), oracle.Pyramid(I1)
    n_waves = 4
    n_easy = n_waves * KPW - len(hard)
    allk, allp = np.concatenate([easy[:n_easy], hard]), np.concatenate([epri[:n_easy], hpri])
    for nl in (0, 3):
        want = _oracle_each(oracle, o0, o1, allk, allp, nl)
        assert want[1][:n_easy].mean() > 0.9 and not want[1][-2:].any()   # easy ones track, the flat block does not
        seen = None
        for slots in (STRADDLE, (4, 11), (6, 9)):
            order = np.array([n_easy + (-1 - k) if k < 0 else k for k in _layout(slots, len(hard), n_waves)])
            assert sorted(order) == list(range(len(allk)))
            got = _track_dev(ctx, g0, g1, allk[order], allp[order], nl)
            _assert_same(got, tuple(a[order] for a in want), (nl, slots))
            inv = np.argsort(order)
            by_kp = tuple(a[inv] for a in got)
            if seen is not None:
                for a, b in zip(by_kp, seen):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (nl, slots)
            seen = by_kp


def _saturated_pair():
    """test_fb_klt_saturated_images' right third on the whole image: 0 / 255 vertical stripes (a grey line every 12 rows keeps
    the 2 x 2 system regular) tracked into a constant 255 image, left 250 columns: block noise with a real 1 px shift"""
    rng = np.random.default_rng(51)
    w, h = 752, 480
    blk = np.kron(rng.integers(0, 2, (h // 3 + 1, w // 3 + 1)), np.ones((3, 3)))[:h, :w].astype(np.uint8) * 255
    I0, I1 = blk.copy(), blk.copy()
    I1[:, :250] = np.roll(I0, 1, axis=1)[:, :250]
    xs = np.arange(w)
    I0[:, 250:] = np.where((xs // 3) % 2 == 1, 255, 0).astype(np.uint8)[None, 250:]
    I0[::12, 250:] = 128
    I1[:, 250:] = 255
    return I0, I1


def _widest_lane_partial(I0, kp):
    """largest |b1| share of a three-column lane in the first level-0 iteration of an integer keypoint tracked into the
    constant 255 image from its own position: sum over 9 rows x 3 columns of 32 (255 - I) Ix, Ix = Scharr [3 10 3]' x [-1 0 1]"""
    x, y = int(kp[0]), int(kp[1])
    P = I0[y - 5:y + 6, x - 5:x + 6].astype(np.int64)
    sm = 3 * P[:-2] + 10 * P[1:-1] + 3 * P[2:]
    ix = sm[:, 2:] - sm[:, :-2]
    prod = 32 * (255 - P[1:-1, 1:-1]) * ix
    return max(abs(int(prod[:, 3 * c:3 * c + 3].sum())) for c in range(3))


def test_wide_sum_path_in_the_straddling_groups(three_lanes, oracle):
    """keypoints on the saturated stripes make a lane's share of b1 exceed 2^27, which sends their whole wave through the
    exact f64 three-lane sum: such keypoints in slots 5 and 10 only (block-noise keypoints elsewhere), and in every slot"""
    ctx = three_lanes
    I0, I1 = _saturated_pair()
    g0, g1 = fe.preprocess_image(ctx, I0, use_clahe=False), fe.preprocess_image(ctx, I1, use_clahe=False)
    o0, o1 = oracle.Pyramid(I0), oracle.Pyramid(I1)
    rng = np.random.default_rng(8)
    n_waves = 3
    cand = np.stack([rng.integers(300, 700, 40), rng.integers(20, 460, 40)], 1).astype(np.float32)
    # a lane whose three columns are exactly one dark stripe sees its two edges cancel: keep the other phases
    stripes = np.array([k for k in cand if _widest_lane_partial(I0, k) > 1 << 27][:2 * n_waves])
    assert len(stripes) == 2 * n_waves
    noise = np.stack([rng.uniform(20, 220, 80), rng.uniform(20, 460, 80)], 1).astype(np.float32)
    more = np.stack([rng.uniform(270, 730, KPW * n_waves), rng.uniform(20, 460, KPW * n_waves)], 1).astype(np.float32)
    order = _layout(STRADDLE, len(stripes), n_waves)
    mixed = np.array([stripes[-1 - k] if k < 0 else noise[k] for k in order], np.float32)
    for nl in (0, 3):
        for kps in (mixed, more):
            want = _oracle_each(oracle, o0, o1, kps, kps, nl)
            _assert_same(_track_dev(ctx, g0, g1, kps, kps, nl), want, nl)
    assert want[2].sum() > 0


B, NPI = 3, 150   # images of a batch, keypoints per image (no multiple of 21)


@pytest.fixture(scope="module")
def batch3(three_lanes, oracle):
    """three 233 x 121 image pairs (previous -> current, and left -> right with 6 px disparity), batched pyramids and one
    pyramid per image, the oracle's pyramids, keypoints and ground truth per image"""
    ctx = three_lanes
    w, h = 233, 121
    prev, cur, right = [], [], []
    for b in range(B):
        tex = synth.base_texture(h + 40, w + 40, seed=70 + b)
        prev.append(np.ascontiguousarray(tex[10:10 + h, 10:10 + w]).astype(np.uint8))
        cur.append(np.ascontiguousarray(tex[11:11 + h, 12:12 + w]).astype(np.uint8))       # content moves by (-2, -1)
        right.append(np.ascontiguousarray(tex[10:10 + h, 16:16 + w]).astype(np.uint8))     # ... by (-6, 0)
    def batched(imgs):
        im = fe.Images(ctx, B, w, h)
        for b in range(B):
            im.upload(b, imgs[b])
        return fe.preprocess_images(ctx, im, use_clahe=False), im
    gp, gc, gr = batched(prev), batched(cur), batched(right)
    single = [[fe.preprocess_image(ctx, I[b], use_clahe=False) for b in range(B)] for I in (prev, cur, right)]
    orc = [[oracle.Pyramid(I[b]) for b in range(B)] for I in (prev, cur, right)]
    kps = [synth.grid_keypoints(NPI, w, h, border=12, seed=90 + b) for b in range(B)]
    return dict(g=(gp[0], gc[0], gr[0]), keep=(gp[1], gc[1], gr[1]), single=single, orc=orc, kps=kps)


def _priors(kps, shift, mix, b):
    """per image: image 0 easy priors, image 1 priors 25 px off (fewer than 33 % track on two levels), image 2 easy;
    mix: 'images' = 70 / 30, all-prior and no-prior by image; 'all' / 'none' / 'mixed' = the whole call"""
    gt = kps - np.float32(shift)
    pri, has = synth.make_priors(kps, gt, sigma=25.0 if b == 1 else 1.0, seed=20 + b)
    if mix == "all" or (mix == "images" and b == 1):
        pri, has = synth.make_priors(kps, gt, frac_prior=1.1, sigma=25.0 if b == 1 else 1.0, seed=20 + b)
    elif mix == "none" or (mix == "images" and b == 2):
        pri, has = kps.copy(), np.zeros(len(kps), np.uint8)
    return pri, has


def _two_stage_dev(ctx, g0, g1, kps, pri, has, img_idx, nb):
    n = len(kps)
    d_o, d_s, d_r = ctx.empty((n, 2), np.float32), ctx.empty((n,), np.uint8), ctx.to_device(np.full(nb, -1, np.int32))
    d_i = None if img_idx is None else ctx.to_device(img_idx)
    fe.FeatureTracker(ctx, 30, 0.01).kltTracking_dev(g0, g1, 9, 3, 30.0, 0.5, ctx.to_device(kps), ctx.to_device(pri),
                                                    ctx.to_device(has), d_o, d_s, n, d_i, d_r, None)
    ctx.synchronize()
    return d_o.get(), d_s.get().astype(bool), d_r.get()


@pytest.mark.parametrize("mix", ["images", "all", "none", "mixed"])
def test_two_stage_tracking_on_a_batch(three_lanes, oracle, batch3, mix):
    """kltTracking on three images with an image index per keypoint (interleaved, so that the keypoints of a wave belong to
    different images): per image the result equals the oracle's klt_tracking_frame keyed by keypoint, including the 33 %
    flag -- raised for image 1 whose priors are 25 px off, which also re-tracks its failures from the keypoint -- and
    equals the same image tracked alone (batch independence)"""
    ctx = three_lanes
    pr = [_priors(batch3["kps"][b], (2, 1), mix, b) for b in range(B)]
    perm = np.random.default_rng(3).permutation(B * NPI)
    kps = np.concatenate(batch3["kps"])[perm]
    pri, has = np.concatenate([p[0] for p in pr])[perm], np.concatenate([p[1] for p in pr])[perm]
    idx = np.repeat(np.arange(B, dtype=np.int32), NPI)[perm]
    out, st, p3p = _two_stage_dev(ctx, batch3["g"][0], batch3["g"][1], kps, pri, has, idx, B)
    for b in range(B):
        rows = np.flatnonzero(idx == b)
        rows = rows[np.argsort(perm[rows])]           # back to the image's own keypoint order
        eo, es, ep3p = oracle.klt_tracking_frame(batch3["orc"][0][b], batch3["orc"][1][b], batch3["kps"][b], pr[b][0], pr[b][1])
        assert bool(p3p[b]) == ep3p, (mix, b)
        assert ep3p == (b == 1 and mix != "none"), (mix, b)
        assert np.array_equal(st[rows], es.astype(bool)), (mix, b)
        assert np.array_equal(out[rows].view(np.uint32), eo.view(np.uint32)), (mix, b)
        so, ss, sp = _two_stage_dev(ctx, batch3["single"][0][b], batch3["single"][1][b], batch3["kps"][b], pr[b][0], pr[b][1], None, 1)
        assert bool(sp[0]) == ep3p and np.array_equal(ss, st[rows]) and np.array_equal(so.view(np.uint32), out[rows].view(np.uint32)), (mix, b)
    assert mix == "none" or st[idx == 0].mean() > 0.8


@pytest.mark.parametrize("mix", ["images", "all", "none", "mixed"])
def test_stereo_matching_on_a_batch(three_lanes, oracle, batch3, mix):
    """left -> right matching (no 33 % rule: failures are re-tracked from the updated prior) on the same batch, against the
    oracle's stereo_matching per image, and against the image matched alone"""
    ctx = three_lanes
    pr = [_priors(batch3["kps"][b], (6, 0), mix, b) for b in range(B)]
    perm = np.random.default_rng(4).permutation(B * NPI)
    kps = np.concatenate(batch3["kps"])[perm]
    pri, has = np.concatenate([p[0] for p in pr])[perm], np.concatenate([p[1] for p in pr])[perm]
    idx = np.repeat(np.arange(B, dtype=np.int32), NPI)[perm]
    trk = fe.FeatureTracker(ctx, 30, 0.01)
    n = len(kps)
    d_o, d_s = ctx.empty((n, 2), np.float32), ctx.empty((n,), np.uint8)
    trk.stereoMatching_dev(batch3["g"][0], batch3["g"][2], 9, 3, 30.0, 0.5, ctx.to_device(kps), ctx.to_device(pri),
                           ctx.to_device(has), d_o, d_s, n, ctx.to_device(idx), None, True, None)
    ctx.synchronize()
    out, st = d_o.get(), d_s.get().astype(bool)
    for b in range(B):
        rows = np.flatnonzero(idx == b)
        rows = rows[np.argsort(perm[rows])]
        eo, es = oracle.stereo_matching(batch3["orc"][0][b], batch3["orc"][2][b], batch3["kps"][b], pr[b][0], pr[b][1])
        assert np.array_equal(st[rows], es), (mix, b)
        assert np.array_equal(out[rows].view(np.uint32), eo.view(np.uint32)), (mix, b)
        so, ss = trk.stereoMatching(batch3["single"][0][b], batch3["single"][2][b], 9, 3, 30.0, 0.5, batch3["kps"][b], pr[b][0], pr[b][1])
        assert np.array_equal(ss, st[rows]) and np.array_equal(so.view(np.uint32), out[rows].view(np.uint32)), (mix, b)
    assert st[idx == 0].mean() > 0.5
