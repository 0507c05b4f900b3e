"""A CU share (ov2_ctx_create_cu, ov2slam_amd/csrc/ctx.hip): the three kernel streams of a context masked to n compute
units.  A share changes where kernels run and nothing they compute, so a tracking call and a local-BA job on contexts
with n = 1 and n = 8 must give the bytes an unmasked context gives; the mask HIP reports is the one ov2_cu_mask_build
makes; the default rule of ov2_ctx_create_ex masks a normal-priority context only beside a live high-priority one; the
matcher's automatic sizing follows the share; and a masked (blocking) stream and the default stream do not lock up."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, frontend as fe, local_ba, synth, synth_ba
from test_stereo_lists_gpu import Call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
XCDS = int(re.search(r"#define\s+OV2_CU_MASK_XCDS\s+(\d+)", HEADER).group(1))
W, H = 96, 64
N_KPS, N_NO_PRIOR, N_FAIL = 70, 23, 8      # 70 keypoints: three waves of 21 and a partial fourth
INVALID = -1


def _device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _effective(total, mask):
    """compute units a mask runs on: an XCD the mask gives no bit runs on all of its own (include/ov2slam_hip.h)"""
    bits = ((mask[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)[:total]
    return sum(int(bits[x::XCDS].sum()) or len(bits[x::XCDS]) for x in range(XCDS))


def tracking_case():
    """(I0, I1, kps, prior, has_prior): 96 x 64, content moved by (2, 1); 23 keypoints without a prior, one row of 8 whose
    priors are 12 px off (the CPU oracle: most of them fail on two levels and are re-tracked on the full pyramid), the
    rest 0.5 px off"""
    tex = synth.base_texture(H + 40, W + 40, seed=W)
    I0 = np.ascontiguousarray(tex[10:10 + H, 10:10 + W]).astype(np.uint8)
    I1 = np.ascontiguousarray(tex[11:11 + H, 12:12 + W]).astype(np.uint8)
    rng = np.random.default_rng(3)
    kps = np.stack([rng.uniform(14, W - 14, N_KPS), rng.uniform(14, H - 14, N_KPS)], 1).astype(np.float32)
    kps[:N_FAIL, 0] = np.linspace(16, W - 16, N_FAIL)
    kps[:N_FAIL, 1] = 31.5                                        # the row of failures
    pri = kps - np.float32([2.0, 1.0]) + rng.normal(0, 0.5, kps.shape).astype(np.float32)
    pri[:N_FAIL, 0] += np.float32(12.0) * np.where(np.arange(N_FAIL) % 2, 1, -1).astype(np.float32)
    has = np.ones(N_KPS, np.uint8)
    has[N_FAIL:N_FAIL + N_NO_PRIOR] = 0
    perm = rng.permutation(N_KPS)
    return I0, I1, np.ascontiguousarray(kps[perm]), np.ascontiguousarray(pri[perm]), np.ascontiguousarray(has[perm])


def _track(c):
    """one two-stage tracking call on context c: positions, status, work words, P3P flag"""
    I0, I1, kps, pri, has = tracking_case()
    g = fe.preprocess_image(c, I0, use_clahe=False), fe.preprocess_image(c, I1, use_clahe=False)
    call = Call(c, kps, pri, has, batch=1).track(g)
    c.synchronize()
    out = list(call.get()) + [call.d_r.get()]
    for p in g:
        p.release()
    return out


def _ba_job(c):
    """set-up -> solve -> update of one small window on a device map of context c: every array the three stages leave"""
    w = synth_ba.make_window(6, 80, inv_depth=True)
    m = DM.DeviceMap.from_problem(c, w, isobs="newest")
    try:
        views = DM.setup_batch(c, [m], nmin_covscore=5, calib_l=synth_ba.K_L)
        assert not views[0].aborted and views[0].n_res > 0
        pcs, rcs = DM.problems_of(views, w, True)
        o = local_ba.default_options()
        assert c.lib.ov2_ba_solve_batch_dev(c.h, 1, pcs, C.byref(o), rcs) == 0
        f = DM.fetch_view(c, views[0], True)
        upd = DM.update_batch(c, [m], views, cur_kfid=[m.newkf])[0]
        for k in ("removed_obs", "stereo_off"):      # lists the update kernels append to through a counter: a set, in any order
            upd[k] = upd[k][np.lexsort((upd[k][:, 1], upd[k][:, 0]))]
        assert len(upd["removed_obs"]) > 0
        d = m.download()
        out = []
        for part in (f, upd, d):
            out += [np.ascontiguousarray(part[k]) for k in sorted(part) if isinstance(part[k], np.ndarray)]
        return out
    finally:
        m.close()


def _same(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


@pytest.fixture(scope="module")
def unmasked():
    """the outputs of both calls on a context without a share, computed once"""
    c = fe.Context(0, cu_share=0)
    try:
        assert c.get_cu_share() == 0
        trk, ba = _track(c), _ba_job(c)
    finally:
        c.close()
    out, st, work, _ = trk
    _, _, _, _, has = tracking_case()
    n = len(has)
    assert st.any() and (work[n:][has == 0] != 0).all()      # the no-prior list ran on the full pyramid
    assert (work[n:][has != 0] != 0).any()                    # and failures of the two-level pass were re-tracked
    assert (work[:n][has != 0] != 0).all()
    return trk, ba


@pytest.mark.parametrize("n", [1, 8, 64])
def test_reported_mask_is_the_built_mask(n):
    total = _device_cus()
    words = (total + 31) // 32
    for layout in (fe.CU_LAYOUT_SPREAD, fe.CU_LAYOUT_PACKED):
        c = fe.Context(0, cu_share=n, cu_layout=layout)
        try:
            assert c.get_cu_share() == n
            assert np.array_equal(c.get_cu_mask(words), fe.cu_mask_build(total, n, layout)), (n, layout)
        finally:
            c.close()


@pytest.mark.parametrize("n", [1, 8])
def test_outputs_equal_the_unmasked_context(unmasked, n):
    c = fe.Context(0, cu_share=n)
    try:
        _same(_track(c), unmasked[0], ("tracking", n))
        _same(_ba_job(c), unmasked[1], ("local BA", n))
    finally:
        c.close()


def test_refusals():
    lib, total = fe._lib.load(), _device_cus()
    h = C.c_void_p()
    for dev, high, n, layout in ((0, 1, 8, 0), (0, 0, -1, 0), (0, 0, total, 0), (0, 0, total + 1, 1), (0, 0, 8, 2), (0, 0, 8, -1)):
        assert lib.ov2_ctx_create_cu(dev, high, n, layout, C.byref(h)) == INVALID, (high, n, layout)
        assert not h.value
    assert lib.ov2_ctx_create_cu(0, 0, 8, 0, None) == INVALID
    assert lib.ov2_ctx_get_cu_share(None) == -1
    with pytest.raises(fe._lib.Ov2Error):
        fe.Context(0, high_priority=True, cu_share=8)
    hi = fe.Context(0, high_priority=True, cu_share=0)          # high priority without a share is ov2_ctx_create_ex's context
    try:
        assert hi.get_cu_share() == 0 and hi.get_wave_prio() == fe.WAVE_PRIO_HIGH
        assert lib.ov2_ctx_get_cu_mask(hi.h, 0, (C.c_uint32 * 1)()) == INVALID
    finally:
        hi.close()


def _expected_default(total):
    """(share, layout) the default rule hands out in THIS process: the header's constants, or the environment's"""
    n = int(re.search(r"#define\s+OV2_WORKER_CUS_DEFAULT\s+(\d+)", HEADER).group(1))
    lay = re.search(r"#define\s+OV2_WORKER_CU_LAYOUT_DEFAULT\s+(\w+)", HEADER).group(1)
    lay = {"OV2_CU_LAYOUT_SPREAD": 0, "OV2_CU_LAYOUT_PACKED": 1}.get(lay, lay)
    n = int(os.environ.get("OV2_WORKER_CUS", n))
    lay = int(os.environ.get("OV2_WORKER_CU_LAYOUT", lay))
    return (n if 0 < n < total else 0), lay


def _default_rule(total, n, layout):
    """the four situations of the rule, the default being (n, layout)"""
    words = (total + 31) // 32
    alone = fe.Context(0)
    assert alone.get_cu_share() == 0                             # a plain context alone on the device
    hi = fe.Context(0, high_priority=True)
    beside = fe.Context(0)
    assert hi.get_cu_share() == 0 and alone.get_cu_share() == 0  # the high one is never masked; the older one stays as it was
    assert beside.get_cu_share() == n                            # created while the high-priority context lives
    if n:
        assert np.array_equal(beside.get_cu_mask(words), fe.cu_mask_build(total, n, layout))
    hi2 = fe.Context(0, high_priority=True)
    hi.close()
    still = fe.Context(0)
    assert still.get_cu_share() == n                             # one of two high-priority contexts is left
    hi2.close()
    after = fe.Context(0)
    assert after.get_cu_share() == 0                             # none is left
    assert beside.get_cu_share() == n                            # a context keeps the share it was created with
    for c in (alone, beside, still, after):
        c.close()


def test_default_rule_in_this_process():
    total = _device_cus()
    _default_rule(total, *_expected_default(total))


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import test_cu_share_gpu as T
from ov2slam_amd import frontend as fe
total = T._device_cus()
n, layout = int(sys.argv[2]), int(sys.argv[3])
T._default_rule(total, n if 0 < n < total else 0, layout)
if n:
    # the blocking-stream ordering: a masked context with work in flight and work on the legacy default stream
    hi = fe.Context(0, high_priority=True)
    c = fe.Context(0)
    assert c.get_cu_share() == n
    I0, I1, kps, pri, has = T.tracking_case()
    g = fe.preprocess_image(c, I0, use_clahe=False), fe.preprocess_image(c, I1, use_clahe=False)
    calls = [T.Call(c, kps, pri, has, batch=1) for _ in range(4)]
    x = torch.arange(1 << 20, device="cuda", dtype=torch.float32)
    for k in calls:
        k.track(g)                       # enqueued, nothing synchronised
    s = float((x * 2).sum().item())      # default stream, while the masked streams hold work
    for k in calls:
        k.track(g)
    c.synchronize()
    torch.cuda.synchronize()
    assert s == float(np.arange(1 << 20, dtype=np.float64).sum() * 2)
    ref = [a.copy() for a in calls[0].get()]
    for k in calls[1:]:
        T._same(list(k.get()), ref, "repeat")
    c.close(); hi.close()
print("CHILD OK")
"""


@pytest.mark.parametrize("n,layout", [(0, 0), (16, 0), (16, 1)])
def test_environment_override_in_a_child_process(n, layout):
    """OV2_WORKER_CUS / OV2_WORKER_CU_LAYOUT are read once per process, so each setting gets a process of its own: 0 switches
    the rule off, 16 hands 16 compute units in the asked layout to the context created beside a high-priority one.  With a
    share, the child also keeps tracking calls in flight on the masked (blocking) streams around a torch reduction on the
    default stream: both finish and give their results, within the child's time limit"""
    env = dict(os.environ, OV2_WORKER_CUS=str(n), OV2_WORKER_CU_LAYOUT=str(layout))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(n), str(layout)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_matcher_sizing_follows_the_share():
    """ov2_knn_lanes_for: the fewest lanes of 1, 4, 16 that give every compute unit a 256-thread workgroup, else 64 -- with
    the compute units the context runs on in place of the device's"""
    total = _device_cus()

    def rule(cus, q):
        for lanes in (1, 4, 16):
            if q * lanes >= 256 * cus:
                return lanes
        return 64

    sizes = (0, 1, 100, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 5000, 16384, 60000, 65536, 300000)
    for share, cus in ((8, 8), (64, 64), (0, total), (1, _effective(total, fe.cu_mask_build(total, 1)))):
        c = fe.Context(0, cu_share=share)
        try:
            got = [c.lib.ov2_knn_lanes_for(c.h, q) for q in sizes]
            assert got == [rule(cus, q) for q in sizes], (share, cus, got)
            c.set_knn_lanes(4)
            assert c.lib.ov2_knn_lanes_for(c.h, 100) == 4          # a forced mapping is reported as it is
            assert c.lib.ov2_knn_lanes_for(c.h, -1) == -1
        finally:
            c.close()
    assert [rule(8, q) for q in sizes] != [rule(total, q) for q in sizes]
    assert fe._lib.load().ov2_knn_lanes_for(None, 10) == -1
