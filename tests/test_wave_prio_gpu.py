"""The wave priority a context hands its kernels (ov2_ctx_set_wave_prio, ov2wave::set_wave_prio in csrc/ov2_wave.h) changes
no result.  What could go wrong is a guard that is not wave-uniform, a kernel argument shifted by the new one, or a scalar
register clobbered by the selection, so every kernel that takes the level runs at level 0 and at non-zero levels on the
smallest shapes that reach all its paths: every output is bitwise the one of level 0, and level 0 is compared with the
oracle.  Tracking cases are those of test_stereo_lists_gpu (lists A, B and C, see there)."""
import os
import re

import numpy as np
import pytest

from ov2slam_amd import frontend as fe, local_ba, synth, synth_ba
from test_stereo_lists_gpu import Batch2, Call, Pools, H, W, _check_stereo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FE_LEVELS = (0, 1, 3)
# n = 1, 20, 21, 22, 43 keypoints as (list B, list C, list A that tracks): around the 21 keypoints of a three-lane wave
SHAPES = {1: (0, 0, 1), 20: (7, 3, 10), 21: (7, 4, 10), 22: (8, 4, 10), 43: (15, 8, 20)}


@pytest.fixture(scope="module")
def pools(ctx, oracle, stream):
    return Pools(ctx, oracle, stream, 0)


@pytest.fixture(scope="module")
def batch2(ctx, oracle, stream, pools):
    return Batch2(ctx, oracle, stream, pools)


@pytest.fixture
def level(ctx):
    """sets the wave priority of the shared context; whatever a test leaves is put back"""
    before = ctx.get_wave_prio()
    try:
        yield ctx.set_wave_prio
    finally:
        ctx.set_wave_prio(before)
        ctx.set_klt_lanes(0)


def _same(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


def test_setter_and_getter(ctx):
    high = int(re.search(r"#define\s+OV2_WAVE_PRIO_HIGH\s+(\d+)", open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()).group(1))
    assert 0 <= high <= 3 and fe.WAVE_PRIO_HIGH == high
    hi, lo = fe.Context(0, high_priority=True), fe.Context(0)
    try:
        assert hi.get_wave_prio() == high     # a fresh high-priority context reports the default level
        assert lo.get_wave_prio() == 0        # a fresh normal-priority one reports 0
        for c in (hi, lo):
            for lv in (0, 1, 2, 3):
                c.set_wave_prio(lv)
                assert c.get_wave_prio() == lv
            for bad in (-1, 4):
                assert c.lib.ov2_ctx_set_wave_prio(c.h, bad) == -1    # OV2_ERR_INVALID
                with pytest.raises(Exception):
                    c.set_wave_prio(bad)
                assert c.get_wave_prio() == 3                          # the level stays
    finally:
        hi.close()
        lo.close()
    assert ctx.lib.ov2_ctx_set_wave_prio(None, 1) == -1 and ctx.lib.ov2_ctx_get_wave_prio(None) == -1


@pytest.mark.parametrize("clahe,nlvl", [(True, 3), (True, 2), (True, 0), (False, 3)])
def test_pyramid_builds(ctx, oracle, stream, level, clahe, nlvl):
    """one image and a batch of two through every build path: the LUT kernel and the fused level-0 + pyrDown kernel, then
    the two-level pyrDown (4 levels) or the single one (3 levels); the tiled CLAHE kernel (1 level); the plain level-0
    kernel, the two-level and the single pyrDown (no CLAHE).  Downloading a level writes the gradient planes (level_kernel)"""
    imgs = [stream.left(0), stream.right(3)]
    assert imgs[0].shape == (H, W)

    def planes(p, b):
        out = []
        for l in range(nlvl + 1):
            img, grad = p.level(l, b)[:2]
            out += [img, grad]
        return out

    res = {}
    for lv in FE_LEVELS:
        level(lv)
        one = fe.preprocess_image(ctx, imgs[0], use_clahe=clahe, nklt_pyr_lvl=nlvl)
        im = fe.Images(ctx, 2, W, H)
        for b, I in enumerate(imgs):
            im.upload(b, I)
        two = fe.preprocess_images(ctx, im, use_clahe=clahe, nklt_pyr_lvl=nlvl)
        res[lv] = planes(one, 0) + planes(two, 0) + planes(two, 1)
        one.release()
        two.release()
    for b, I in ((0, imgs[0]), (1, imgs[0]), (2, imgs[1])):     # level 0 against the oracle
        o = oracle.Pyramid(oracle.clahe(I) if clahe else I, 9, nlvl)
        for l in range(nlvl + 1):
            oi, og = o.level(l)[:2]
            gi, gg = res[0][2 * (b * (nlvl + 1) + l)], res[0][2 * (b * (nlvl + 1) + l) + 1]
            assert np.array_equal(gi, oi) and np.array_equal(gg, og), (b, l)
    for lv in FE_LEVELS[1:]:
        _same(res[lv], res[0], (clahe, nlvl, lv))


@pytest.mark.parametrize("gl,n", [(3, 1), (3, 20), (3, 21), (3, 22), (3, 43), (8, 22), (16, 22)])
def test_tracking_and_stereo_calls(ctx, oracle, pools, level, gl, n):
    """a stereo call (compaction, first launch = list A, second launch = lists B and C, gate) and a two-stage tracking call
    (first launch = lists A and B, second = list C) on the same keypoints"""
    nb, nc, na = SHAPES[n]
    assert nb + nc + na == n
    case = pools.case(oracle, nb, nc, na)
    kps, pri, has = case[:3]
    eo, es, ep = oracle.klt_tracking_frame(*pools.o, kps, pri, has)
    ctx.set_klt_lanes(gl)
    res = {}
    for lv in FE_LEVELS:
        level(lv)
        s, t = Call(ctx, kps, pri, has), Call(ctx, kps, pri, has, batch=1)
        s.stereo(pools.g)
        t.track(pools.g)
        ctx.synchronize()
        if lv == 0:
            _check_stereo(s, case, (gl, n))
            out, st, _ = t.get()
            assert np.array_equal(st.astype(bool), es.astype(bool)) and np.array_equal(out.view(np.uint32), eo.view(np.uint32))
            assert bool(t.d_r.get()[0]) == ep
        res[lv] = list(s.get()) + list(t.get()) + [t.d_r.get()]
    for lv in FE_LEVELS[1:]:
        _same(res[lv], res[0], (gl, n, lv))


def test_forward_backward_call(ctx, oracle, pools, level):
    """ov2_klt_track_fb_dev (klt_fb_kernel): 22 keypoints, three lanes and sixteen"""
    kps, pri = pools.case(oracle, 8, 4, 10)[:2]
    eo, es, _ = oracle.fb_klt_tracking(*pools.o, kps, pri, 9, 3, 30.0, 0.5, 30, 0.01)
    trk = fe.FeatureTracker(ctx, 30, 0.01)
    for gl in (3, 16):
        ctx.set_klt_lanes(gl)
        res = {}
        for lv in FE_LEVELS:
            level(lv)
            out, st = trk.fbKltTracking(*pools.g, 9, 3, 30.0, 0.5, kps, pri)
            res[lv] = [out, st]
        assert np.array_equal(res[0][1], es.astype(bool)) and np.array_equal(res[0][0].view(np.uint32), eo.view(np.uint32)), gl
        for lv in FE_LEVELS[1:]:
            _same(res[lv], res[0], (gl, lv))


def test_batched_stereo_and_detector(ctx, batch2, level):
    """the stereo call on a batch of two followed by ov2_detect_grid_batch_dev on the left pyramid (mask, work list,
    min-eigenvalue cells, assembly, sub-pixel refinement)"""
    cell, cap = 35, 2 * (W // 35) * (H // 35)
    cur = [k for k, _, _ in batch2.per]
    d_cur = ctx.to_device(np.concatenate(cur).astype(np.float32))
    d_cur_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(cur)]))
    n_cur = sum(len(c) for c in cur)
    res = {}
    for lv in FE_LEVELS:
        level(lv)
        d_th = ctx.to_device(np.full(2, 0.001, np.float64))
        d_nout, d_out = ctx.to_device(np.full(2, -7, np.int32)), ctx.to_device(np.zeros((2, cap, 2), np.float32))
        call = batch2.stereo_call(ctx)
        call.stereo(batch2.g[:2])
        fe.detect_grid_batch_dev(ctx, batch2.g[0], cell, 1, d_th, n_cur, d_cur, d_cur_img, None, d_nout, d_out, cap)
        ctx.synchronize()
        if lv == 0:
            batch2.check_stereo(call, lv)
        res[lv] = list(call.get()) + [a.get() for a in (d_nout, d_out, d_th)]
    assert (res[0][3] > 0).all()
    for lv in FE_LEVELS[1:]:
        _same(res[lv], res[0], lv)


def test_fast_detector_cells(ctx, stream, level):
    """the FAST cells of the grid detector (det_fast_kernel), one image"""
    p = fe.preprocess_image(ctx, stream.left(0))
    cur = synth.grid_keypoints(20)
    res = {}
    for lv in FE_LEVELS:
        level(lv)
        ex = fe.FeatureExtractor(ctx, nmaxdist=35, dmaxquality=0.001)     # a fresh one: the detector adapts its threshold
        res[lv] = [ex.detectGridFAST(p, cur), np.array([ex.nfast_th_])]
    assert len(res[0][0]) > 0
    for lv in FE_LEVELS[1:]:
        _same(res[lv], res[0], lv)


def test_solver_batch(ctx, level):
    """ov2_ba_solve_batch_dev on two windows of 8 keyframes and 300 landmarks (inverse depth) at levels 0 and 3: poses,
    landmarks, chi2, flags and the iteration log bitwise equal"""
    res = {}
    for lv in (0, 3):
        level(lv)
        Ps = [synth_ba.make_window(8, 300, inv_depth=True, seed=s) for s in (1, 2)]
        Ds = [local_ba.DeviceBaProblem(ctx, p) for p in Ps]
        Rd = local_ba.Optimizer(ctx).localBA_batch_dev(Ds)
        arrays, logs = [], []
        for D, r in zip(Ds, Rd):
            arrays += [np.ascontiguousarray(a) for a in D.download()]
            logs.append((r.n_log, r.n_log_robust, r.termination, r.l2_termination, r.l2_done, r.initial_cost, r.final_cost,
                         r.l2_initial_cost, r.l2_final_cost, r.n_outliers_pass1, r.n_outliers_pass2,
                         [(r.log[i].cost, r.log[i].radius) for i in range(r.n_log)]))
        assert all(l[0] > 1 for l in logs)
        res[lv] = (arrays, logs)
    _same(res[3][0], res[0][0], "solver")
    assert res[3][1] == res[0][1]
