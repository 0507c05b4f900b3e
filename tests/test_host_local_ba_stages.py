"""The local BA of the C++ host mirror in its stages -- set-up (ov2h_local_ba_setup), update (ov2h_local_ba_update) -- with
map edits between them, as the reference's other threads make them while Optimizer::localBA solves without the map lock
(src/optimizer.cpp:741).  CPU only: the update reads the MapPoint / Frame objects as they are at that moment, and the
whole-map export (ov2h_map_export) is what the device tests compare the device tables against."""
import numpy as np
import pytest

from ov2slam_amd import device_map as DM
from ov2slam_amd import host_map, synth_ba


def _window(inv_depth, seed=23):
    P = synth_ba.make_window(12, 700, inv_depth=inv_depth, seed=seed)
    P.res_uv = P.res_uv.astype(np.float32).astype(np.float64)   # Keypoint::unpx_ is float
    if P.lm_anchor_uv is not None:
        P.lm_anchor_uv = P.lm_anchor_uv.astype(np.float32).astype(np.float64)
    return P


def _observers(state):
    by_lm = {}
    for k, l in state[2]:
        by_lm.setdefault(l, []).append(k)
    return {l: sorted(v) for l, v in by_lm.items()}


def _keys(a):
    return list(zip(a["res_type"].tolist(), a["res_kfid"].tolist(), a["res_lmid"].tolist()))


@pytest.mark.parametrize("inv_depth", [True, False])
def test_export_and_update_without_flags_keep_the_map(inv_depth):
    P = _window(inv_depth)
    hm = host_map.HostMap(P)
    kfs0, lms0, obs0 = hm.export()
    assert sorted(kfs0) == list(range(len(P.pose))) and sorted(lms0) == list(range(len(P.lm)))
    kf, lm, _, st, _ = DM.observations_of(P)
    assert obs0 == {(int(k), int(l)): 2 * int(s) for k, l, s in zip(kf, lm, st)}
    for k in kfs0:
        assert np.array_equal(kfs0[k], P.pose[k])
    a = hm.setup_local_ba()
    hm.update_local_ba(np.zeros(len(a["res_type"]), np.uint8))
    kfs1, lms1, obs1 = hm.export()
    assert obs1 == obs0 and sorted(lms1) == sorted(lms0)
    for k in kfs0:   # solved poses written back = the set-up's
        assert np.array_equal(kfs1[k], kfs0[k])
    for l in lms0:   # every isobs_ is set: nothing is culled; inverse depth -> world point round trip
        assert lms1[l][1] == lms0[l][1]
        assert np.allclose(lms1[l][0], lms0[l][0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("inv_depth", [True, False])
def test_flagged_blocks_remove_and_demote_observations(inv_depth):
    P = _window(inv_depth, seed=5)
    hm = host_map.HostMap(P)
    a = hm.setup_local_ba()
    keys = _keys(a)
    rng = np.random.default_rng(1)
    flags = (rng.random(len(keys)) < 0.05).astype(np.uint8)
    left = {(k, l) for (t, k, l), f in zip(keys, flags) if f and t in (DM.T.L_XYZ, DM.T.L_INV)}
    right = {(k, l) for (t, k, l), f in zip(keys, flags) if f and t not in (DM.T.L_XYZ, DM.T.L_INV)} - left
    assert left and right
    _, lms0, obs0 = hm.export()
    hm.update_local_ba(flags)
    _, lms1, obs1 = hm.export()
    assert not (left & set(obs1))
    assert {o for o in right if o[1] in lms1} <= set(obs1) and all(obs1[o] == 0 for o in right if o in obs1)
    assert set(obs0) - set(obs1) == left | {o for o in obs0 if o[1] not in lms1}
    # the current frame's observations that were flagged cleared MapPoint::isobs_ (removeObsFromCurFrameById)
    for k, l in left:
        if k == len(P.pose) - 1 and l in lms1:
            assert not lms1[l][1] & DM.LM_OBS


@pytest.mark.parametrize("inv_depth", [True, False])
def test_culling_reads_the_observers_of_the_moment(inv_depth):
    """landmarks with two old observers and isobs_ cleared are culled by the update (fewer than 3 observers, older than
    newkf - 3, src/optimizer.cpp:808-813) -- unless a keyframe added between set-up and update observes them too; removing
    the observation that anchors a landmark moves MapPoint::kfid_ and, with inverse depth, the keyframe whose pose and pixel
    turn the solved inverse depth into the new world point (:822-838)"""
    P = _window(inv_depth, seed=9)
    newkf = len(P.pose) - 1
    maps = [host_map.HostMap(P) for _ in range(2)]
    state = maps[0].export()
    obs_by = _observers(state)
    twos = [l for l, ks in obs_by.items() if len(ks) >= 3 and ks[1] < newkf - 3 and newkf not in ks][:12]
    assert len(twos) == 12
    for h in maps:
        for l in twos:
            for k in obs_by[l][2:]:
                h.remove_obs(k, l)
            h.set_isobs(l, 0)
    a = [h.setup_local_ba() for h in maps]
    assert _keys(a[0]) == _keys(a[1])
    twos_local = [l for l in twos if l in set(a[0]["lm_lmid"].tolist())]
    assert len(twos_local) >= 6
    saved = twos_local[::2]
    T = np.ascontiguousarray(P.pose[newkf])
    maps[1].add_keyframe_obs(newkf + 1, T, saved, np.full((len(saved), 2), 300.0, np.float32))
    # anchors that go away mid-solve: the oldest observer of a landmark with enough observers left
    movers = [l for l, ks in obs_by.items() if len(ks) >= 4 and l not in twos and l in set(a[0]["lm_lmid"].tolist())][:10]
    for l in movers:
        maps[1].remove_obs(obs_by[l][0], l)
    for h, pb in zip(maps, a):
        h.update_local_ba(np.zeros(len(pb["res_type"]), np.uint8))
    s0, s1 = maps[0].export(), maps[1].export()
    assert not set(twos_local) & set(s0[1])                    # culled
    assert set(saved) <= set(s1[1])                            # a third observer arrived in time
    assert not (set(twos_local) - set(saved)) & set(s1[1])
    assert all((newkf + 1, l) in s1[2] for l in saved)
    if inv_depth:   # the moved anchor: Twc(new anchor) * (K^-1 [u v 1] / rho), rho as solved for the old anchor
        K = P.calib_l
        lm_ix = {int(l): i for i, l in enumerate(a[1]["lm_lmid"])}
        kf, lm, un, _, _ = DM.observations_of(P)
        for l in movers:
            k = obs_by[l][1]
            u, v = un[np.flatnonzero((kf == k) & (lm == l))[0]]
            z = 1.0 / a[1]["lm"][lm_ix[l], 0]
            pc = np.array([z * (u - K[2]) / K[0], z * (v - K[3]) / K[1], z])
            want = synth_ba.quat_to_rot(P.pose[k, 3:]) @ pc + P.pose[k, :3]
            assert np.allclose(s1[1][l][0], want, rtol=1e-12, atol=1e-12), l
    else:
        for l in movers:
            assert s1[1][l][0] == s0[1][l][0]


def test_append_obs_joins_an_existing_keyframe():
    P = _window(True, seed=3)
    hm = host_map.HostMap(P)
    kfs, lms, obs = hm.export()
    k = len(P.pose) - 2
    new = [l for l in sorted(lms) if (k, l) not in obs][:5]
    hm.append_obs(k, new, np.full((5, 2), 100.0, np.float32), stereo=[1, 0, 1, 0, 0], ruv=np.full((5, 2), 90.0, np.float32))
    _, lms1, obs1 = hm.export()
    assert set(obs1) - set(obs) == {(k, l) for l in new}
    assert [obs1[(k, l)] for l in new] == [2, 0, 2, 0, 0]
    with pytest.raises(AssertionError):   # one observation per (keyframe, landmark)
        hm.append_obs(k, new[:1], np.zeros((1, 2), np.float32))
