"""The lazy join of the keyframe detector chain (ov2_ctx_set_kf_lazy_join, ov2slam_amd/csrc/detect.hip): the detector call
leaves its chain pending on the side stream, the first call that needs the main stream behind it joins, and a tracking or
stereo call whose arrays are proven apart from the chain's runs beside it.  Every case runs the same calls with the eager
join (the detector call joins its chain itself) and with the lazy join on one context and requires np.array_equal on every
output of every call; the detector outputs are also the oracle's.  Which path a case took is read from
ov2_ctx_kf_join_stats, never from timing.

Shapes: a batch of 2 images of 96 x 80 (four pyramid levels at window 9), cell 16 (6 x 5 cells: 3 x 3, 3 x 3, 2 x 3 and
2 x 3 cells of the four colours), 48 existing keypoints and 48 tracked keypoints with interleaved image indices."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe

pytestmark = pytest.mark.gpu

W, H, B = 96, 80, 2
WIN, NLVL = 9, 3
CELL, MINEIG, TH0 = 16, 1, 0.001
CAP = 2 * (W // CELL) * (H // CELL)
N = 48                      # existing keypoints of the detector = tracked keypoints: the hazard cases alias the two sets
COUNTERS = ("started", "conflict", "default", "sync", "covered", "eager", "pyr_waits")


def _crop(img, x0, y0=150):
    return np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W])


class Rig:
    """two contexts of its own (the cases switch the join of the context they run on) and the images of every case"""

    def __init__(self, stream):
        self.ctx, self.mctx = fe.Context(0), fe.Context(0)
        self.raw_a = [_crop(stream.left(0), 200), _crop(stream.left(0), 330)]
        self.raw_b = [_crop(stream.left(0), 202), _crop(stream.left(0), 331)]     # the same scene moved by 2 and 1 px
        self.raw_r = [_crop(stream.right(0), 196), _crop(stream.right(0), 327)]
        self.raw_x = [[_crop(stream.left(3 * k), 240 + 10 * k), _crop(stream.left(3 * k), 400 + 10 * k)] for k in range(1, 6)]
        self.ims = {k: self.images(self.ctx, v) for k, v in (("a", self.raw_a), ("b", self.raw_b), ("r", self.raw_r))}
        self.ims_x = [self.images(self.ctx, v) for v in self.raw_x]
        rng = np.random.default_rng(5)
        self.cur = np.stack([rng.uniform(2, W - 2, N), rng.uniform(2, H - 2, N)], 1).astype(np.float32)
        self.cur_img = (np.arange(N) % B).astype(np.int32)                        # interleaved image indices
        self.cur_valid = (rng.uniform(size=N) < 0.9).astype(np.uint8)
        self.kps = np.stack([rng.uniform(14, W - 14, N), rng.uniform(14, H - 14, N)], 1).astype(np.float32)
        self.has = (rng.uniform(size=N) < 0.7).astype(np.uint8)
        self.pri = (self.kps + rng.uniform(-1.5, 1.5, self.kps.shape)).astype(np.float32)
        self.trk = fe.FeatureTracker(self.ctx, 30, 0.01)
        self.mtrk = fe.FeatureTracker(self.mctx, 30, 0.01)

    @staticmethod
    def images(ctx, raws):
        ims = fe.Images(ctx, len(raws), W, H)
        for b, r in enumerate(raws):
            ims.upload(b, r)
        return ims

    def pyr(self, which, ctx=None):
        ims = self.ims[which] if isinstance(which, str) else self.ims_x[which]
        return fe.preprocess_images(ctx or self.ctx, ims, False, 3.0, WIN, NLVL)

    def close(self):
        self.mctx.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig(stream):
    r = Rig(stream)
    yield r
    r.close()


@pytest.fixture(scope="module")
def want(rig, oracle):
    """the oracle's detector result on the two images of set a, computed once: [(corners, threshold)] per image"""
    out = []
    for b in range(B):
        sel = (rig.cur_img == b) & (rig.cur_valid != 0)
        out.append(oracle.detect_single_scale(rig.raw_a[b], CELL, rig.cur[sel], TH0))
    assert sum(len(c) for c, _ in out) > 0
    return out


class Arrays:
    """every device array of a case, allocated BEFORE the first detector call: an allocation enqueues a fill on the main
    stream and would join a pending chain"""

    def __init__(self, rig):
        ctx = rig.ctx
        self.d_th = ctx.to_device(np.full(B, TH0, np.float64))
        self.d_nout = ctx.to_device(np.full(B, -7, np.int32))
        self.d_out = ctx.to_device(np.zeros((B, CAP, 2), np.float32))
        self.d_cur = ctx.to_device(rig.cur)
        self.d_cur_img = ctx.to_device(rig.cur_img)
        self.d_cur_valid = ctx.to_device(rig.cur_valid)
        self.d_kps, self.d_pri, self.d_has = ctx.to_device(rig.kps), ctx.to_device(rig.pri), ctx.to_device(rig.has)
        self.d_idx = ctx.to_device(rig.cur_img)
        self.d_txy, self.d_tst = ctx.to_device(np.zeros((N, 2), np.float32)), ctx.to_device(np.zeros(N, np.uint8))
        self.d_sxy, self.d_sst = ctx.to_device(np.zeros((N, 2), np.float32)), ctx.to_device(np.zeros(N, np.uint8))
        self.d_p3p, self.d_work = ctx.to_device(np.zeros(B, np.int32)), ctx.to_device(np.zeros(2 * N, np.uint32))
        self.d_misc = ctx.to_device(np.zeros(16, np.float32))


def _detect(rig, A, pyr, cell=CELL, d_th=None, d_nout=None, d_out=None):
    fe.detect_grid_batch_dev(rig.ctx, pyr, cell, MINEIG, d_th or A.d_th, N, A.d_cur, A.d_cur_img, A.d_cur_valid,
                             d_nout or A.d_nout, d_out or A.d_out, CAP)


def _track(rig, A, prev, cur, d_kps=None, d_txy=None, d_tst=None, trk=None):
    (trk or rig.trk).kltTracking_dev(prev, cur, WIN, NLVL, 30.0, 0.5, d_kps or A.d_kps, A.d_pri, A.d_has, d_txy or A.d_txy,
                                     d_tst or A.d_tst, N, A.d_idx, A.d_p3p, A.d_work)


def _stereo(rig, A, left, right):
    rig.trk.stereoMatching_dev(left, right, WIN, NLVL, 30.0, 0.5, A.d_kps, A.d_pri, A.d_has, A.d_sxy, A.d_sst, N, A.d_idx,
                               None, True, None)


def _det_results(A):
    return dict(count=A.d_nout.get(), corners=A.d_out.get().view(np.uint32), thresh=A.d_th.get())


def _trk_results(A):
    return dict(txy=A.d_txy.get().view(np.uint32), tst=A.d_tst.get(), p3p=A.d_p3p.get(), work=A.d_work.get())


def _check_oracle(res, want):
    for b, (corners, th) in enumerate(want):
        assert res["count"][b] == len(corners), b
        assert np.array_equal(res["corners"][b, :len(corners)], corners.view(np.uint32)), b
        assert res["thresh"][b] == float(th), b


def _drain(rig):
    """takes every pooled pyramid buffer out of the pool (all of them have finished: the context was synchronised) and
    returns the handles to hold: the next buffer released is then the only one a build can reuse"""
    held = []
    while rig.ctx.pyr_pool_stats()["pooled"] and len(held) < 32:
        held.append(rig.pyr("b"))
    assert rig.ctx.pyr_pool_stats()["pooled"] == 0
    return held


def _both(rig, run, pyr_waits=False):
    """run(lazy) with the eager join, then with the lazy join; run returns (results, {stage: stats}).  Every array of the
    two results must be equal; returns the lazy results and the lazy run's counters relative to the run's start.  The
    pyr_waits counter is kept only for the cases that empty the pool first: elsewhere a build may take a buffer that an
    earlier case released under its chain."""
    ctx, outs = rig.ctx, []
    counters = COUNTERS if pyr_waits else COUNTERS[:-1]
    for lazy in (False, True):
        ctx.set_kf_lazy_join(lazy)
        try:
            ctx.synchronize()
            s0 = ctx.kf_join_stats()
            assert s0["pending"] == 0
            res, stages = run(lazy)
            ctx.synchronize()
            stages["end"] = ctx.kf_join_stats()
            assert stages["end"]["pending"] == 0
            outs.append((res, {k: {c: v[c] - s0[c] for c in counters} | {"pending": v["pending"]} for k, v in stages.items()}))
        finally:
            ctx.set_kf_lazy_join(True)
    (eager, es), (lazy, ls) = outs
    assert eager.keys() == lazy.keys()
    for k in eager:
        assert np.array_equal(eager[k], lazy[k]), k
    assert es["end"]["eager"] == es["end"]["started"] and es["end"]["pending"] == 0     # the eager join never leaves a chain
    assert all(es["end"][c] == 0 for c in ("conflict", "default", "sync", "covered"))
    assert ls["end"]["eager"] == 0
    return lazy, ls


def test_a_outputs_read_at_once(rig, want):
    """the read-back is an ordinary use of the main stream: it joins"""
    def run(lazy):
        A, p = Arrays(rig), rig.pyr("a")
        _detect(rig, A, p)
        after = rig.ctx.kf_join_stats()
        res = _det_results(A)
        return res, dict(call=after, read=rig.ctx.kf_join_stats())

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["call"]["pending"] == 1 and st["call"]["started"] == 1 and st["call"]["default"] == 0
    assert st["read"]["pending"] == 0 and st["read"]["default"] == 1
    assert st["end"] == dict(started=1, conflict=0, default=1, sync=0, covered=0, eager=0, pending=0)


def test_b_stereo_detector_tracking_on_disjoint_arrays(rig, want):
    """the flagship order: nothing joins before the final synchronise, and the tracking call's results are the eager ones"""
    def run(lazy):
        A, left, right, nxt = Arrays(rig), rig.pyr("a"), rig.pyr("r"), rig.pyr("b")
        _stereo(rig, A, left, right)
        _detect(rig, A, left)
        _track(rig, A, left, nxt)
        after = rig.ctx.kf_join_stats()
        rig.ctx.synchronize()
        synced = rig.ctx.kf_join_stats()
        res = dict(_det_results(A), **_trk_results(A), sxy=A.d_sxy.get().view(np.uint32), sst=A.d_sst.get())
        return res, dict(tracked=after, synced=synced)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert res["tst"].sum() > 0
    assert st["tracked"] == dict(started=1, conflict=0, default=0, sync=0, covered=0, eager=0, pending=1)
    assert st["synced"] == dict(started=1, conflict=0, default=0, sync=1, covered=0, eager=0, pending=0)
    assert st["end"] == st["synced"]


def test_b2_stereo_call_beside_a_pending_chain(rig, want):
    """a stereo call (tracking launches and the gate) on arrays apart from the chain's leaves it pending as well"""
    def run(lazy):
        A, left, right = Arrays(rig), rig.pyr("a"), rig.pyr("r")
        _detect(rig, A, left)
        _stereo(rig, A, left, right)
        after = rig.ctx.kf_join_stats()
        return dict(_det_results(A), sxy=A.d_sxy.get().view(np.uint32), sst=A.d_sst.get()), dict(stereo=after)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["stereo"]["pending"] == 1 and st["stereo"]["conflict"] == 0 and st["stereo"]["default"] == 0


@pytest.mark.parametrize("case", ["c_reads_corners", "d_writes_keypoints", "e_writes_flags"])
def test_cde_range_conflicts(rig, want, case):
    """c: the tracked keypoints are the detector's corners (read after write); d: the tracked positions land on the
    detector's keypoints, e: the statuses on its validity flags (write after read): each joins by range conflict"""
    def run(lazy):
        A, p, nxt = Arrays(rig), rig.pyr("a"), rig.pyr("b")
        _detect(rig, A, p)
        if case == "c_reads_corners":
            _track(rig, A, p, nxt, d_kps=A.d_out)      # the first 48 rows of the corner block
        elif case == "d_writes_keypoints":
            _track(rig, A, p, nxt, d_txy=A.d_cur)
        else:
            _track(rig, A, p, nxt, d_tst=A.d_cur_valid)
        after = rig.ctx.kf_join_stats()
        res = dict(_det_results(A), **_trk_results(A), cur=A.d_cur.get().view(np.uint32), valid=A.d_cur_valid.get())
        return res, dict(tracked=after)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["tracked"] == dict(started=1, conflict=1, default=0, sync=0, covered=0, eager=0, pending=0)
    if case == "d_writes_keypoints":
        assert not np.array_equal(res["cur"], rig.cur.view(np.uint32))      # the tracking call did overwrite them


@pytest.mark.parametrize("between", ["upload", "copy", "pnp"])
def test_f_other_entry_points_join_by_default(rig, want, between):
    def run(lazy):
        A, p = Arrays(rig), rig.pyr("a")
        extra = {}
        if between == "pnp":
            from ov2slam_amd import synth_ba
            from ov2slam_amd.multi_view_geometry import MultiViewGeometry
            q, mvg = synth_ba.make_pnp(60, seed=2), MultiViewGeometry(rig.ctx)
        _detect(rig, A, p)
        if between == "upload":
            A.d_misc.set(np.arange(16, dtype=np.float32))
        elif between == "copy":
            A.d_txy.copy_from(A.d_cur)
        else:
            ok, T, idx = mvg.ceresPnP(q["unpx"], q["wpts"], q["Twc0"], 5, 5.9915, True, True, *q["K"])
            extra = dict(pnp_T=np.asarray(T).view(np.uint64), pnp_out=np.asarray(idx))
        after = rig.ctx.kf_join_stats()
        return dict(_det_results(A), misc=A.d_misc.get(), txy=A.d_txy.get(), **extra), dict(between=after)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["between"] == dict(started=1, conflict=0, default=1, sync=0, covered=0, eager=0, pending=0)


@pytest.mark.parametrize("ring", [1, 3])
def test_g_pyramid_released_under_a_pending_chain(rig, want, ring):
    """the pyramid the chain reads is released at once, then ring + 1 builds of the same geometry from other images: the
    build that reuses the buffer waits for the chain.  The pool is emptied first, so it holds that buffer alone when the
    builds start and the first build takes it -- at once at depth 1; at depth 3 only if its readers have finished, otherwise
    it allocates, which the pool's counters tell."""
    ctx, allocated, waited = rig.ctx, {}, {}

    def run(lazy):
        A = Arrays(rig)
        ctx.set_pyr_ring(ring)
        drained = _drain(rig)
        p = rig.pyr("a")
        pool0, w0 = ctx.pyr_pool_stats(), ctx.kf_join_stats()["pyr_waits"]      # behind the builds that emptied the pool
        assert pool0["pooled"] == 0
        _detect(rig, A, p)
        p.release()
        held = []
        for k in range(ring + 1):
            q = rig.pyr(k)
            if ring > 1:
                q.release()
            else:
                held.append(q)
        after = ctx.kf_join_stats()
        allocated[lazy] = ctx.pyr_pool_stats()["allocated"] - pool0["allocated"]
        waited[lazy] = after["pyr_waits"] - w0
        res = _det_results(A)
        for q in held + drained:
            q.release()
        return res, dict(built=after)

    try:
        res, st = _both(rig, run, pyr_waits=True)
    finally:
        ctx.set_pyr_ring(3)
    _check_oracle(res, want)
    assert st["built"]["pending"] == 1 and st["built"]["default"] == 0 and st["built"]["conflict"] == 0
    assert waited[False] == 0
    if ring == 1:
        assert waited[True] == 1 and allocated[True] == ring
    else:
        assert waited[True] == 1 or (waited[True] == 0 and allocated[True] >= 1)


def test_h_two_detector_calls_with_no_call_between(rig, want, oracle):
    """the second chain runs behind the first on the side stream; on the same arrays it covers the first (one join for
    both), and its thresholds are the ones the first adapted"""
    def run(lazy):
        A, p = Arrays(rig), rig.pyr("a")
        _detect(rig, A, p)
        first = rig.ctx.kf_join_stats()
        _detect(rig, A, p)
        second = rig.ctx.kf_join_stats()
        return _det_results(A), dict(first=first, second=second)

    res, st = _both(rig, run)
    for b, (_, th) in enumerate(want):      # the oracle's second call: the thresholds of the first feed it
        sel = (rig.cur_img == b) & (rig.cur_valid != 0)
        corners, th2 = oracle.detect_single_scale(rig.raw_a[b], CELL, rig.cur[sel], float(th))
        assert res["count"][b] == len(corners) and res["thresh"][b] == float(th2)
        assert np.array_equal(res["corners"][b, :len(corners)], corners.view(np.uint32))
    assert st["first"]["pending"] == 1 and st["first"]["started"] == 1
    assert st["second"] == dict(started=2, conflict=0, default=0, sync=0, covered=1, eager=0, pending=1)
    assert st["end"] == dict(started=2, conflict=0, default=1, sync=0, covered=1, eager=0, pending=0)


def test_h2_second_chain_on_other_arrays(rig, want):
    """a second chain that writes other arrays does not stand for the first: a tracking call on the first chain's corners
    must still come behind the first chain"""
    def run(lazy):
        A, p, nxt = Arrays(rig), rig.pyr("a"), rig.pyr("b")
        d_th2 = rig.ctx.to_device(np.full(B, TH0, np.float64))
        d_nout2 = rig.ctx.to_device(np.full(B, -7, np.int32))
        d_out2 = rig.ctx.to_device(np.zeros((B, CAP, 2), np.float32))
        _detect(rig, A, p)
        _detect(rig, A, p, d_th=d_th2, d_nout=d_nout2, d_out=d_out2)
        _track(rig, A, p, nxt, d_kps=A.d_out)
        res = dict(_det_results(A), **_trk_results(A), count2=d_nout2.get(), corners2=d_out2.get().view(np.uint32), thresh2=d_th2.get())
        return res, {}

    res, st = _both(rig, run)
    _check_oracle(res, want)
    _check_oracle(dict(count=res["count2"], corners=res["corners2"], thresh=res["thresh2"]), want)
    assert st["end"]["started"] == 2 and st["end"]["covered"] == 1


def test_i_synchronize_completes_a_pending_chain(rig, want):
    def run(lazy):
        A, p, nxt = Arrays(rig), rig.pyr("a"), rig.pyr("b")
        _detect(rig, A, p)
        rig.ctx.synchronize()
        synced = rig.ctx.kf_join_stats()
        _track(rig, A, p, nxt, d_kps=A.d_out)      # would conflict with a chain still pending
        return dict(_det_results(A), **_trk_results(A)), dict(synced=synced)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["synced"] == dict(started=1, conflict=0, default=0, sync=1, covered=0, eager=0, pending=0)
    assert st["end"] == st["synced"]


def test_j_failed_argument_check_after_a_valid_call(rig, want):
    """the failing call enqueues nothing and leaves the first call's chain as it was: pending, and joined by the read-back"""
    def run(lazy):
        A, p = Arrays(rig), rig.pyr("a")
        _detect(rig, A, p)
        with pytest.raises(Exception, match="cell size"):
            _detect(rig, A, p, cell=4)
        failed = rig.ctx.kf_join_stats()
        return _det_results(A), dict(failed=failed)

    res, st = _both(rig, run)
    _check_oracle(res, want)
    assert st["failed"] == dict(started=1, conflict=0, default=0, sync=0, covered=0, eager=0, pending=1)
    assert st["end"] == dict(started=1, conflict=0, default=1, sync=0, covered=0, eager=0, pending=0)


@pytest.mark.parametrize("last", ["owner", "foreign"])
def test_k_foreign_release_under_a_pending_chain(rig, want, last):
    """the keyframe's pyramid is also read by a tracking call on another context and released from there
    (ov2_pyr_release_from) while the owner's chain is pending; either release may be the last one.  A build at ring depth 1
    then reuses the buffer and must wait for the foreign reader and for the chain"""
    ctx, mctx, waited = rig.ctx, rig.mctx, {}

    def run(lazy):
        A = Arrays(rig)
        m_kps, m_pri, m_has, m_idx = (mctx.to_device(x) for x in (rig.kps, rig.pri, rig.has, rig.cur_img))
        m_xy, m_st, m_p3p = mctx.to_device(np.zeros((N, 2), np.float32)), mctx.to_device(np.zeros(N, np.uint8)), mctx.to_device(np.zeros(B, np.int32))
        ctx.set_pyr_ring(1)
        drained = _drain(rig)
        p, nxt = rig.pyr("a"), rig.pyr("b")
        w0 = ctx.kf_join_stats()["pyr_waits"]
        _detect(rig, A, p)
        kfp = p.retain()
        rig.mtrk.kltTracking_dev(kfp, nxt, WIN, NLVL, 30.0, 0.5, m_kps, m_pri, m_has, m_xy, m_st, N, m_idx, m_p3p, None)
        if last == "foreign":
            p.release()
            kfp.release_from(mctx)
        else:
            kfp.release_from(mctx)
            p.release()
        q = rig.pyr(0)
        after = ctx.kf_join_stats()
        waited[lazy] = after["pyr_waits"] - w0
        mctx.synchronize()
        res = dict(_det_results(A), mxy=m_xy.get().view(np.uint32), mst=m_st.get())
        for x in [q, nxt] + drained:
            x.release()
        return res, dict(built=after)

    try:
        res, st = _both(rig, run, pyr_waits=True)
    finally:
        ctx.set_pyr_ring(3)
    _check_oracle(res, want)
    assert res["mst"].sum() > 0
    assert st["built"]["pending"] == 1 and waited == {False: 0, True: 1}


def test_switching_the_join_with_a_chain_pending(rig, want):
    """both setters join a pending chain before they change the setting"""
    ctx = rig.ctx
    for setter in (ctx.set_kf_lazy_join, ctx.set_kf_overlap):
        A, p = Arrays(rig), rig.pyr("a")
        ctx.synchronize()
        s0 = ctx.kf_join_stats()
        _detect(rig, A, p)
        assert ctx.kf_join_stats()["pending"] == 1
        try:
            setter(False)
            s1 = ctx.kf_join_stats()
            assert s1["pending"] == 0 and s1["default"] == s0["default"] + 1
        finally:
            setter(True)
        _check_oracle(_det_results(A), want)


def test_host_pointer_form_returns_complete_results(rig, want):
    """ov2_detect_grid_batch stages through the context and synchronises: no chain is pending behind it"""
    ctx = rig.ctx
    p = rig.pyr("a")
    th = np.full(B, TH0, np.float64)
    cur = [rig.cur[(rig.cur_img == b) & (rig.cur_valid != 0)] for b in range(B)]
    got = fe.detect_grid_batch(ctx, p, CELL, MINEIG, th, cur)
    assert ctx.kf_join_stats()["pending"] == 0
    for b, (corners, t) in enumerate(want):
        assert np.array_equal(got[b].view(np.uint32), corners.view(np.uint32)) and th[b] == float(t)
