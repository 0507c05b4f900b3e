"""ov2_map_pose_graph_update_batch (csrc/map.hip): the update stage of Optimizer::localPoseGraph (reference
src/optimizer.cpp:2476-2577) on the device map mirrors, against the C++ host stage (Optimizer::applyLocalPoseGraph with a
mirror attached, flushed) and against the numpy checker (tests/loop_close_ref.py).

Maps: synth_filter.make_map at (21, 60) and (40, 1200) -- one workgroup and ~25 workgroups of rows per scan.  In those maps
every landmark has an observer older than the three newest keyframes, so none is anchored at a keyframe younger than the
new keyframe nk - 4; `with_younger` appends eight 3D landmarks that only the three younger keyframes see (the rest of the
map is make_map's, row for row), so that the younger branch of the landmark scan has work.
Chain: keyframes 5 .. nk - 4, each pose perturbed by se3_exp(N(0, 0.01)) in numpy -- no solve involved.

Bar against the host stage: every integer and state column exact, poses and points BITWISE equal (the kernels use the
SE(3) product / inverse / apply of the host mirror's SE3 in its order, f64, contraction off on both sides).
Bar against numpy: the same set of moved landmarks, poses and points to 1e-12 m (scene scale <= 20 m)."""
import numpy as np
import pytest
from scipy.linalg import expm

import loop_close_ref as R
from ov2slam_amd import device_map as DM, host_map, synth_filter
from test_oracle_pg import hat6

pytestmark = pytest.mark.gpu
SHAPES = [(21, 60), (40, 1200)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def with_younger(m, n_extra=8):
    """a copy of the map with n_extra more 3D landmarks, seen by the three newest keyframes only"""
    nk, nl = m["n_kf"], m["n_lm"]
    rng = np.random.default_rng(1000 + nk)
    kf, lm = [], []
    for i in range(n_extra):
        a = nk - 3 + i % 3
        kf.append(a); lm.append(nl + i)
        if a != nk - 1:
            kf.append(nk - 1); lm.append(nl + i)
    obs_kf = np.concatenate([m["obs_kf"], np.array(kf, np.int32)])
    obs_lm = np.concatenate([m["obs_lm"], np.array(lm, np.int32)])
    uv = np.stack([rng.uniform(8, m["w"] - 8, len(kf)), rng.uniform(8, m["h"] - 8, len(kf))], 1).astype(np.float32)
    obs_uv = np.concatenate([m["obs_uv"], uv])
    o = np.lexsort((obs_lm, obs_kf))
    one = np.ones(n_extra, np.uint8)
    X = np.stack([rng.uniform(-2, 2 + 0.1 * nk, n_extra), rng.uniform(-1.5, 1.5, n_extra), rng.uniform(2, 9, n_extra)], 1)
    return dict(m, n_lm=nl + n_extra, obs_kf=obs_kf[o], obs_lm=obs_lm[o], obs_uv=obs_uv[o],
                lm_3d=np.concatenate([m["lm_3d"], one]), lm_kp3d=np.concatenate([m["lm_kp3d"], one]),
                lm_isobs=np.concatenate([m["lm_isobs"], one]), lm_xyz=np.vstack([m["lm_xyz"], X]))


_maps = {}


def the_map(nk, nl, seed=None):
    key = (nk, nl, nk if seed is None else seed)
    if key not in _maps:
        _maps[key] = with_younger(synth_filter.make_map(nk, nl, seed=key[2]))
    return _maps[key]


def the_chain(m, seed=None):
    """(newkf, kfids 5 .. nk - 4, their perturbed poses n x 7)"""
    nk = m["n_kf"]
    rng = np.random.default_rng(nk if seed is None else seed)
    ids = np.arange(5, nk - 3, dtype=np.int32)
    T = np.stack([R.pose7(R.mat(m["poses"][k]) @ expm(hat6(rng.normal(0, 0.01, 6)))) for k in ids])
    return nk - 4, ids, T


class _Borrowed:
    """a borrowed ov2_map* with DeviceMap's download()"""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.lib, h
        self._p = DM.DeviceMap._p
        self.download = lambda: DM.DeviceMap.download(self)


def device_result(ctx, m, chain):
    """(header, canonical state, download) of the device form on a freshly built mirror"""
    newkf, ids, T = chain
    dm = DM.DeviceMap.from_filter_map(ctx, m)
    try:
        before = dm.download()
        hdr = dm.pose_graph_update_batch(newkf=[newkf], chain_kfid=[ids], chain_Twc=[T])[0]
        after = dm.download()
    finally:
        dm.close()
    return hdr, DM.canonical_state(after), before, after


_dev = {}


def dev(ctx, nk, nl):
    if (nk, nl) not in _dev:
        m = the_map(nk, nl)
        _dev[(nk, nl)] = device_result(ctx, m, the_chain(m))
    return _dev[(nk, nl)]


def _bits(state):
    """canonical state with every double as its bit pattern: == is then bitwise (0.0 vs -0.0, NaN)"""
    kfs, lms, obs = state
    b = lambda t: tuple(np.asarray(t, np.float64).view(np.uint64).tolist())
    return {k: b(v) for k, v in kfs.items()}, {l: (b(p), s) for l, (p, s) in lms.items()}, obs


@pytest.mark.parametrize("nk,nl", SHAPES)
def test_device_form_equals_host_stage(ctx, nk, nl):
    """the host stage with a mirror attached (touchPose / touchMapPoint + flush_device) against the device call on a fresh
    mirror of the same map.  Largest difference measured on these two maps: 0 (bitwise), poses and points."""
    m = the_map(nk, nl)
    newkf, ids, T = the_chain(m)
    hm = host_map.FilterMap(m)
    hm.attach_device(ctx)
    assert hm.apply_local_pose_graph(newkf, ids, T) == 1
    hm.flush_device()
    host = DM.canonical_state(_Borrowed(ctx, hm.device_handle()).download())
    del hm
    hdr, state, _, _ = dev(ctx, nk, nl)
    hk, hl, ho = host
    dk, dl, do = state
    assert set(hk) == set(dk) and set(hl) == set(dl) and ho == do                     # integer columns
    assert {l: s for l, (_, s) in hl.items()} == {l: s for l, (_, s) in dl.items()}   # landmark states
    dpose = max(np.abs(np.array(hk[k]) - np.array(dk[k])).max() for k in hk)
    dpt = max(np.abs(np.array(hl[l][0]) - np.array(dl[l][0])).max() for l in hl)
    print(f"[pg_update {nk},{nl}] max |pose diff| {dpose:.3e}, max |point diff| {dpt:.3e}, header {hdr}")
    assert _bits(host) == _bits(state)


@pytest.mark.parametrize("nk,nl", SHAPES)
def test_device_form_equals_numpy(ctx, nk, nl):
    m = the_map(nk, nl)
    newkf, ids, T = the_chain(m)
    hdr, state, before, after = dev(ctx, nk, nl)
    seen = np.unique(m["obs_lm"])
    ref_map = dict(poses={k: m["poses"][k] for k in range(nk)},
                   points={int(l): (m["lm_xyz"][l] if m["lm_3d"][l] else np.zeros(3)) for l in seen},
                   obs=list(zip(m["obs_kf"].tolist(), m["obs_lm"].tolist())),
                   kp3d=set(np.flatnonzero(m["lm_kp3d"]).tolist()))
    poses, points, mc, my, Tc = R.update(ref_map, newkf, {int(k): t for k, t in zip(ids, T)})
    assert len(mc) > 5 and len(my) > 5
    changed = set(np.flatnonzero((before["lm_xyz"].view(np.uint64) != after["lm_xyz"].view(np.uint64)).any(1)).tolist())
    assert changed == mc | my
    assert hdr["n_lm_moved"] == len(mc) + len(my) and hdr["n_kf_chain"] == len(ids) and hdr["n_kf_younger"] == 3
    kfs, lms, _ = state
    assert set(kfs) == set(poses) and set(lms) == set(points)
    for k, M in poses.items():
        assert np.abs(R.mat(kfs[k]) - M).max() <= 1e-12, k
    for l, p in points.items():
        assert np.abs(np.array(lms[l][0]) - p).max() <= 1e-12, l
    anch = R.anchors(ref_map)
    low = [l for l, a in anch.items() if a < 5]
    assert len(low) > 5
    for l in low:          # anchored below the chain: bit-unchanged
        assert np.array_equal(before["lm_xyz"][l].view(np.uint64), after["lm_xyz"][l].view(np.uint64))
        assert before["lm_state"][l] == after["lm_state"][l]
    for k in range(5):
        assert np.array_equal(before["kf_pose"][k].view(np.uint64), after["kf_pose"][k].view(np.uint64))
    assert np.abs(R.mat(hdr["T_corr"]) - Tc).max() <= 1e-12
    for l in mc | my:      # MapPoint::setPoint: the point is 3D afterwards, the other bits as they were
        assert after["lm_state"][l] == before["lm_state"][l] | DM.LM_3D


def test_batch_of_eight_equals_eight_single_calls(ctx):
    """eight distinct maps in one call, one of them with an empty list (tables untouched, zero header)"""
    shapes = [(21, 60, 1), (24, 200, 2), (40, 1200, 3), (22, 90, 4), (30, 400, 5), (21, 64, 6), (26, 300, 7), (23, 128, 8)]
    ms = [the_map(*s) for s in shapes]
    chains = [the_chain(m, seed=s[2]) for m, s in zip(ms, shapes)]
    empty = 3
    maps = [DM.DeviceMap.from_filter_map(ctx, m) for m in ms]
    try:
        before = DM.canonical_state(maps[empty].download())
        ids = [c[1] if b != empty else np.zeros(0, np.int32) for b, c in enumerate(chains)]
        Ts = [c[2] if b != empty else np.zeros((0, 7)) for b, c in enumerate(chains)]
        res = DM.pose_graph_update_batch(ctx, maps, newkf=[c[0] for c in chains], chain_kfid=ids, chain_Twc=Ts)
        assert (res[empty]["n_kf_chain"], res[empty]["n_kf_younger"], res[empty]["n_lm_moved"]) == (0, 0, 0)
        assert not res[empty]["T_corr"].any()
        assert _bits(DM.canonical_state(maps[empty].download())) == _bits(before)
        for b, (m, c) in enumerate(zip(ms, chains)):
            if b == empty:
                continue
            hdr, state, _, _ = device_result(ctx, m, c)
            assert hdr["n_lm_moved"] == res[b]["n_lm_moved"] > 10 and hdr["n_kf_younger"] == res[b]["n_kf_younger"] == 3
            assert np.array_equal(hdr["T_corr"].view(np.uint64), res[b]["T_corr"].view(np.uint64))
            assert _bits(DM.canonical_state(maps[b].download())) == _bits(state), shapes[b]
        # the asynchronous form (no header) does the same to the tables
        again = DM.DeviceMap.from_filter_map(ctx, ms[0])
        try:
            assert again.pose_graph_update_batch(newkf=[chains[0][0]], chain_kfid=[chains[0][1]], chain_Twc=[chains[0][2]],
                                                 want_header=False) is None
            assert _bits(DM.canonical_state(again.download())) == _bits(DM.canonical_state(maps[0].download()))
        finally:
            again.close()
    finally:
        for dm in maps:
            dm.close()


def test_refusals(ctx):
    m = the_map(21, 60)
    newkf, ids, T = the_chain(m)
    dm, other = DM.DeviceMap.from_filter_map(ctx, m), DM.DeviceMap.from_filter_map(ctx, m)
    try:
        view = DM.setup_batch(ctx, [dm], calib_l=synth_filter.K4)
        ctl = DM.setup_batch(ctx, [other], calib_l=synth_filter.K4)      # the control: without the call the update runs
        assert DM.update_batch(ctx, [other], ctl, outliers=[np.zeros(ctl[0].n_res, np.uint8)]) is not None
        assert ctx.lib.ov2_map_remove_keyframe(dm.h, 7) == 0
        before = _bits(DM.canonical_state(dm.download()))

        def refused(match, maps=None, newkf_=newkf, ids_=ids, T_=T):
            maps = [dm] if maps is None else maps
            with pytest.raises(Exception, match=match):
                DM.pose_graph_update_batch(ctx, maps, newkf=[newkf_] * len(maps), chain_kfid=[ids_] * len(maps),
                                           chain_Twc=[T_] * len(maps))
            assert _bits(DM.canonical_state(dm.download())) == before

        refused(r"\(-1\).*keyframe 7 is not alive")                                   # a dead chain keyframe
        keep = ids != 7
        ids2, T2 = ids[keep], T[keep]
        refused(r"\(-1\).*ascend", ids_=ids2[::-1].copy(), T_=T2[::-1].copy())         # a list that descends
        refused(r"\(-1\).*ends in keyframe", ids_=ids2[:-1], T_=T2[:-1])               # ... that does not end in newkf
        refused(r"\(-1\).*twice", maps=[dm, dm], ids_=ids2, T_=T2)                     # a map named twice
        refused(r"\(-1\).*not alive", newkf_=10 ** 6, ids_=ids2, T_=T2)                # newkf out of range
        bad = ids2.copy()
        bad[0] = -1
        refused(r"\(-1\).*not alive", ids_=bad, T_=T2)                                 # a listed id out of range
        # a valid call ends what the set-up made before it can be updated from
        hdr = DM.pose_graph_update_batch(ctx, [dm, other], newkf=[newkf, newkf], chain_kfid=[ids2, ids],
                                         chain_Twc=[T2, T])
        assert hdr[0]["n_kf_chain"] == len(ids2) and hdr[1]["n_kf_chain"] == len(ids)
        with pytest.raises(Exception, match=r"\(-1\).*no set-up to update from"):
            DM.update_batch(ctx, [dm], view)
    finally:
        dm.close()
        other.close()
