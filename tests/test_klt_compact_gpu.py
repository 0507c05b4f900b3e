"""The list compaction in front of the two tracking launches (klt_compact_kernel, ov2slam_amd/csrc/klt.hip): a thread
takes eight keypoints, a wave 512 consecutive ones and a workgroup 2048, with one atomic per list and workgroup.
kltTracking_dev and stereoMatching_dev with a work-word buffer on a 160 x 120 crop of the stream, call sizes
around a thread's eight keypoints and a workgroup's 2048, and has_prior patterns that put every keypoint, none, every
other one, a random half and one block of eight across the first workgroup boundary on list A.

Positions (float32 bit patterns), status and the 33 % flag are compared with the oracle's klt_tracking_frame /
stereo_matching on the same arrays.  The work words say which list a keypoint was on: iters[i] holds the two-level pass of a
keypoint of list A, iters[n + i] the full-pyramid pass of a keypoint of list B or of a failure of list A, low 16 bits =
LK iterations, zero where the keypoint takes no part; the oracle, one keypoint at a time, gives the iteration counts."""
import numpy as np
import pytest

from ov2slam_amd import frontend as fe

pytestmark = pytest.mark.gpu

W, H = 160, 120
WIN, NLVL = 9, 3
N_MAX = 4097
SIZES = (1, 7, 8, 9, 63, 65, 511, 513, 2047, 2048, 2049, 4097)   # around a thread's eight, a slot's 64, a wave's 512, a workgroup's 2048
PATTERNS = ("none", "all", "alternating", "random", "straddle")


def _pattern(name, n):
    i = np.arange(n)
    if name == "none":
        return np.zeros(n, np.uint8)
    if name == "all":
        return np.ones(n, np.uint8)
    if name == "alternating":
        return (i & 1).astype(np.uint8)
    if name == "random":
        return (np.random.default_rng(n).uniform(size=n) < 0.5).astype(np.uint8) * 7   # any non-zero byte is a prior
    return ((i >= 2044) & (i < 2052)).astype(np.uint8)   # eight keypoints, four on each side of the first workgroup's end


def _each(oracle, o0, o1, kps, pri, nl):
    """the oracle one keypoint at a time: (forward result, status, LK iterations) of each"""
    out, st, it = np.empty_like(kps), np.zeros(len(kps), bool), np.zeros(len(kps), np.int64)
    for i in range(len(kps)):
        o, s, t = oracle.fb_klt_tracking(o0, o1, kps[i:i + 1], pri[i:i + 1], WIN, nl, 30.0, 0.5, 30, 0.01)
        out[i], st[i], it[i] = o[0], bool(s[0]), t
    return out, st, it


class Scene:
    """a 160 x 120 crop of the stream's left image and the same crop three pixels to the right (a rectified pair and a frame
    pair at once), N_MAX keypoints all over the image with priors about a pixel off the truth, and what the oracle says
    about each keypoint alone: the two-level pass from the prior, and the full-pyramid pass from the failed forward result,
    from the keypoint itself and from the prior.  A case is a prefix of the keypoints: the tables are made once"""

    def __init__(self, ctx, oracle, stream):
        L = stream.left(0)
        I0 = np.ascontiguousarray(L[150:150 + H, 300:300 + W])
        I1 = np.ascontiguousarray(L[150:150 + H, 303:303 + W])
        self.g = fe.preprocess_image(ctx, I0, use_clahe=False), fe.preprocess_image(ctx, I1, use_clahe=False)
        self.o = oracle.Pyramid(I0), oracle.Pyramid(I1)
        rng = np.random.default_rng(11)
        self.kps = np.stack([rng.uniform(2, W - 2, N_MAX), rng.uniform(2, H - 2, N_MAX)], 1).astype(np.float32)
        self.pri = (self.kps + np.float32([-3.0, 0.0]) + rng.normal(0, 1.0, self.kps.shape)).astype(np.float32)
        self.pri[::9] += np.float32(7.0)                      # some priors the two-level pass cannot recover: list C
        self.fwd, self.st_a, self.it_a = _each(oracle, *self.o, self.kps, self.pri, 1)
        fail = ~self.st_a
        assert 100 < fail.sum() < N_MAX // 2, int(fail.sum())
        self.it_fwd = np.zeros(N_MAX, np.int64)
        self.it_fwd[fail] = _each(oracle, *self.o, self.kps[fail], self.fwd[fail], NLVL)[2]
        self.it_own = _each(oracle, *self.o, self.kps, self.kps, NLVL)[2]
        self.it_pri = _each(oracle, *self.o, self.kps, self.pri, NLVL)[2]
        self.cache = {}

    def words(self, has, stereo, drop):
        """(LK iterations of the two-level pass, of the full-pyramid pass, who takes the full-pyramid pass) of a case"""
        n, has = len(has), has != 0
        fail = has & ~self.st_a[:n]
        it_a = np.where(has, self.it_a[:n], 0)
        it_full = np.where(has, 0, (self.it_pri if stereo else self.it_own)[:n])
        it_full[fail] = (self.it_own if drop else self.it_fwd)[:n][fail]
        return it_a, it_full, ~has | fail

    def expect(self, oracle, kind, n, has):
        key = (kind, n, has.tobytes())
        if key not in self.cache:
            if kind == "stereo":
                xy, st = oracle.stereo_matching(*self.o, self.kps[:n], self.pri[:n], has)
                self.cache[key] = xy, np.asarray(st).astype(bool), False
            else:
                xy, st, p3p = oracle.klt_tracking_frame(*self.o, self.kps[:n], self.pri[:n], has)
                self.cache[key] = xy, st.astype(bool), p3p
        return self.cache[key]


@pytest.fixture(scope="module")
def scene(ctx, oracle, stream):
    return Scene(ctx, oracle, stream)


@pytest.fixture
def lanes(ctx):
    def choose(n):
        ctx.set_klt_lanes(n)
    try:
        yield choose
    finally:
        ctx.set_klt_lanes(0)


class Call:
    """the device-resident arguments and outputs of one call, uploaded before anything is enqueued and held until the
    results are read; every output starts from a pattern the call must overwrite.  `shift` puts has_prior at an address
    that is no multiple of eight"""

    def __init__(self, ctx, scene, kind, n, has, shift=0):
        self.kind, self.n, self.has, self.scene = kind, n, has, scene
        self.trk = fe.FeatureTracker(ctx, 30, 0.01)
        self.d_k, self.d_p = ctx.to_device(scene.kps[:n]), ctx.to_device(scene.pri[:n])
        self.d_h = ctx.to_device(np.concatenate([np.full(shift, 1, np.uint8), has, np.full(8, 1, np.uint8)]))
        self.h_ptr = self.d_h.ptr.value + shift if shift else self.d_h
        self.d_o = ctx.to_device(np.full((n, 2), -777.0, np.float32))
        self.d_s = ctx.to_device(np.full(n, 9, np.uint8))
        self.d_w = ctx.to_device(np.full(2 * n, 0xdeadbeef, np.uint32))
        self.d_r = ctx.to_device(np.full(1, -1, np.int32))

    def enqueue(self):
        g = self.scene.g
        if self.kind == "stereo":
            self.trk.stereoMatching_dev(g[0], g[1], WIN, NLVL, 30.0, 0.5, self.d_k, self.d_p, self.h_ptr, self.d_o, self.d_s,
                                        self.n, None, None, True, None, d_iters=self.d_w)
        else:
            self.trk.kltTracking_dev(g[0], g[1], WIN, NLVL, 30.0, 0.5, self.d_k, self.d_p, self.h_ptr, self.d_o, self.d_s,
                                     self.n, None, self.d_r, self.d_w)
        return self

    def check(self, oracle, what):
        n, has, stereo = self.n, self.has, self.kind == "stereo"
        exy, est, ep3p = self.scene.expect(oracle, self.kind, n, has)
        out, st, work = self.d_o.get(), self.d_s.get(), self.d_w.get()
        assert set(np.unique(st)) <= {0, 1}, what
        assert np.array_equal(st.astype(bool), est), what
        assert np.array_equal(out.view(np.uint32), exy.view(np.uint32)), what
        if not stereo:
            assert int(self.d_r.get()[0]) == int(ep3p), what
        it_a, it_full, full = self.scene.words(has, stereo, ep3p)
        w_a, w_full = work[:n], work[n:]
        assert np.array_equal((w_a & 0xffff).astype(np.int64), it_a), what
        assert np.array_equal((w_full & 0xffff).astype(np.int64), it_full), what
        assert np.array_equal(w_a == 0, has == 0), what          # list A = the keypoints with a prior, each once
        assert np.array_equal(w_full == 0, ~full), what          # list B and list C = the rest and the failures
        assert max((w_a >> 16).max(), (w_full >> 16).max()) <= NLVL + 2, what


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_patterns(ctx, oracle, scene, n):
    for kind in ("track", "stereo"):
        for name in PATTERNS:
            call = Call(ctx, scene, kind, n, _pattern(name, n)).enqueue()
            ctx.synchronize()
            call.check(oracle, (kind, n, name))


@pytest.mark.parametrize("gl", [3, 8, 16])
def test_each_mapping(ctx, oracle, scene, lanes, gl):
    lanes(gl)
    for kind in ("track", "stereo"):
        call = Call(ctx, scene, kind, 2049, _pattern("random", 2049)).enqueue()
        ctx.synchronize()
        call.check(oracle, (gl, kind))


def test_calls_back_to_back(ctx, oracle, scene):
    """stereo, tracking, stereo with different lists and nothing synchronised in between: the counter double buffer and the
    zero word serve calls that hand list B to different launches"""
    calls = [Call(ctx, scene, "stereo", 4097, _pattern("random", 4097)), Call(ctx, scene, "track", 2049, _pattern("alternating", 2049)),
             Call(ctx, scene, "stereo", 2047, _pattern("straddle", 2047)), Call(ctx, scene, "track", 4097, _pattern("none", 4097))]
    for c in calls:
        c.enqueue()
    ctx.synchronize()
    for k, c in enumerate(calls):
        c.check(oracle, k)


@pytest.mark.parametrize("shift", [1, 4])
def test_flags_off_an_eight_byte_boundary(ctx, oracle, scene, shift):
    """has_prior inside a larger array, at an address that is no multiple of eight (or of four)"""
    for kind in ("track", "stereo"):
        call = Call(ctx, scene, kind, 2049, _pattern("random", 2049), shift=shift).enqueue()
        ctx.synchronize()
        call.check(oracle, (kind, shift))
