"""The map-point merge (MapManager::mergeMapPoints, reference src/map_manager.cpp:801-882) without a GPU: the checker
(tests/merge_ref.py) on a hand-written map with the expected rows written out, the pair lists of the GPU tests
(tests/test_map_merge_gpu.py) -- a hand-built list that reaches every branch plus a seeded random list per map -- with the
promise that they are not vacuous, and the checker against the C++ host stage (ov2::MapManager::mergeMapPoints on
host_map.FilterMap) after every pair."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ov2slam_amd import synth_filter
import merge_ref as R

MAPS = [(21, 60, 0), (40, 1200, 0)]          # (keyframes, landmarks, seed): 360 and 6082 rows
N_RANDOM = {60: 40, 1200: 300}               # random pairs per map; 300 is more than one 256-wide chunk of a launch
OTHER_SEED = (21, 60, 5)                     # the third map of the batch tests

_cache = {}


def the_map(nk, nl, seed):
    if (nk, nl, seed) not in _cache:
        m = synth_filter.make_map(nk, nl, seed=seed)
        _cache[(nk, nl, seed)] = (m, R.tables_of(m))
    return _cache[(nk, nl, seed)]


def _find(cands, used, k, pred):
    """the first k-tuple of distinct unused landmarks that satisfies pred; it is marked used"""
    free = [l for l in cands if l not in used]
    for t in itertools.permutations(free, k):
        if pred(*t):
            used.update(t)
            return t
    raise AssertionError("the map holds no such landmarks")


def hand_pairs(d):
    """a list that reaches every branch of the stage on the map of tables d.  Returns (pairs (n, 2) int32, cur_obs (n,) uint8,
    names: {what: index or (index, index) into the list})"""
    M = R.build(d)
    O = {l: frozenset(s) for l, s in M["lms"].items()}
    st, L = d["lm_state"], len(d["lm_state"])
    c3 = [l for l in sorted(O) if st[l] & R.LM_3D and O[l]][:160]
    not3d = [l for l in sorted(O) if not st[l] & R.LM_3D]
    dead1, dead2 = L - 2, L - 1
    assert not3d and dead1 not in O and dead2 not in O
    used = set()
    x = c3[0]
    pairs, cur, names = [], [], {}

    def add(name, *ps, cur_obs=0):
        names[name] = len(pairs) if len(ps) == 1 else tuple(range(len(pairs), len(pairs) + len(ps)))
        pairs.extend(ps); cur.extend([cur_obs] * len(ps))

    add("range", (-1, x), (x, L + 5))
    add("same", (x, x))
    add("prev_dead", (dead1, x))
    add("new_dead", (x, dead2))
    add("new_not3d", (x, not3d[0]))
    add("all_moved", _find(c3, used, 2, lambda p, n: not O[p] & O[n]))
    add("mixed", _find(c3, used, 2, lambda p, n: O[p] & O[n] and O[p] - O[n]))
    add("all_conflict", _find(c3, used, 2, lambda p, n: O[p] <= O[n]))
    a, b, c = _find(c3, used, 3, lambda a, b, c: O[a] - O[b] - O[c])
    add("chain", (a, b), (b, c))                  # a row of a that neither b nor c shares a keyframe with moves twice
    add("prev_gone", (a, c))                      # (a -> b), (a -> c): a left the map with the first pair
    a, b, n = _find(c3, used, 3, lambda a, b, n: (O[a] & O[b]) - O[n])
    add("shared", (a, n), (b, n))                 # a keyframe sees a and b: b's row of it stays behind as a conflict
    add("cur", _find(c3, used, 2, lambda p, n: not st[n] & R.LM_OBS), cur_obs=1)
    return np.array(pairs, np.int32), np.array(cur, np.uint8), names


def random_pairs(nl, count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, nl, (count, 2)).astype(np.int32), (rng.random(count) < 0.3).astype(np.uint8)


def full_list(nk, nl, seed):
    """(pairs, cur_obs, names) of a map: the hand-built list, then the random one"""
    d = the_map(nk, nl, seed)[1]
    hp, hc, names = hand_pairs(d)
    rp, rc = random_pairs(nl, N_RANDOM[nl], seed=100 + seed + nl)
    return np.concatenate([hp, rp]), np.concatenate([hc, rc]), names


def test_checker_on_a_hand_written_map():
    """keyframes 0..3; 0 sees {0, 1}, 1 sees {0, 2}, 2 sees {1, 2}, 3 sees {3}; every landmark 3D"""
    kf = np.array([0, 0, 1, 1, 2, 2, 3], np.int32)
    lm = np.array([0, 1, 0, 2, 1, 2, 3], np.int32)
    d = dict(kf_pose=np.zeros((4, 7)), kf_state=np.ones(4, np.uint8), lm_xyz=np.zeros((5, 3)),
             lm_state=np.array([3, 3, 3, 3, 0], np.uint8), obs_kf=kf, obs_lm=lm, obs_flag=np.ones(7, np.uint8),
             obs_uv=np.arange(14.0).reshape(7, 2), obs_ruv=np.zeros((7, 2)))
    M = R.build(d)
    assert R.merge_pair(M, 0, 1) == (R.DONE, 1, 1)            # keyframe 0 holds 1 already; keyframe 1's row moves
    assert M["lms"][1] == {0, 1, 2} and 0 not in M["lms"] and M["tables"]["obs_lm"].tolist() == [0, 1, 1, 2, 1, 2, 3]
    assert R.merge_pair(M, 2, 1) == (R.DONE, 0, 2)            # keyframe 1 holds 1 only since the first pair
    assert R.merge_pair(M, 0, 3) == (R.SKIP_PREV_DEAD, 0, 0)
    assert R.merge_pair(M, 3, 4) == (R.SKIP_NEW_DEAD, 0, 0)
    assert R.merge_pair(M, 3, 3) == (R.SKIP_SAME, 0, 0) and R.merge_pair(M, 3, 5) == (R.SKIP_RANGE, 0, 0)
    assert R.merge_pair(M, 3, 1, cur_obs=True) == (R.DONE, 1, 0)
    assert set(M["row"]) == {(0, 1), (1, 1), (2, 1), (3, 1)} and M["tables"]["lm_state"].tolist() == [0, 7, 0, 0, 0]
    assert R.row_dict(M)[(1, 1)][0] == (4.0, 5.0) and R.row_dict(M)[(3, 1)][0] == (12.0, 13.0)
    assert d["obs_lm"].tolist() == lm.tolist() and d["lm_state"].tolist() == [3, 3, 3, 3, 0]   # the input is left alone
    # taken at once against the first table, (2 -> 1) would have moved keyframe 1's row
    M2 = R.build(d)
    assert R.merge_pair(M2, 2, 1) == (R.DONE, 1, 1)


@pytest.mark.parametrize("nk,nl,seed", MAPS)
def test_lists_reach_every_branch(nk, nl, seed):
    m, d = the_map(nk, nl, seed)
    assert len(m["obs_kf"]) == {60: 360, 1200: 6082}[nl]
    pairs, cur, names = full_list(nk, nl, seed)
    M = R.build(d)
    before = d["lm_state"].copy()
    hdr, status, rec = R.merge_list(M, pairs, cur)
    assert hdr["n_rows_moved"] > 0 and hdr["n_rows_conflict"] > 0 and hdr["n_pairs"] == len(pairs) == hdr["n_merged"] + hdr["n_skipped"]
    assert set(status.tolist()) == {R.DONE, R.SKIP_RANGE, R.SKIP_SAME, R.SKIP_PREV_DEAD, R.SKIP_NEW_DEAD, R.SKIP_NEW_NOT3D}
    i, j = names["range"]
    assert rec[i][0] == rec[j][0] == R.SKIP_RANGE and rec[names["same"]][0] == R.SKIP_SAME
    assert rec[names["prev_dead"]][0] == rec[names["prev_gone"]][0] == R.SKIP_PREV_DEAD
    assert rec[names["new_dead"]][0] == R.SKIP_NEW_DEAD and rec[names["new_not3d"]][0] == R.SKIP_NEW_NOT3D
    s, mv, cf = rec[names["all_moved"]]
    assert s == R.DONE and mv > 0 and cf == 0
    s, mv, cf = rec[names["mixed"]]
    assert s == R.DONE and mv > 0 and cf > 0
    s, mv, cf = rec[names["all_conflict"]]
    assert s == R.DONE and mv == 0 and cf > 0
    i, j = names["chain"]
    assert rec[i][0] == rec[j][0] == R.DONE and max(M["relabels"].values()) >= 2
    i, j = names["shared"]
    assert rec[i][0] == rec[j][0] == R.DONE and pairs[i][1] == pairs[j][1] and rec[j][2] > 0
    i = names["cur"]
    assert rec[i][0] == R.DONE and cur[i] and not before[pairs[i][1]] & R.LM_OBS and M["tables"]["lm_state"][pairs[i][1]] & R.LM_OBS
    # the random part alone holds merges of every kind as well
    tail = rec[len(rec) - N_RANDOM[nl]:]
    assert any(r[1] and not r[2] for r in tail) and any(r[1] and r[2] for r in tail) and any(r[0] == R.DONE and not r[1] for r in tail)


# ---- the C++ host stage, no device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _built():
    import __graft_entry__ as g
    g.build()


def host_merge(hm, p, n):
    from ov2slam_amd import host_map
    L = host_map.lib()
    L.ov2h_map_merge_points.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert L.ov2h_map_merge_points(hm.h, int(p), int(n)) == 0


def without_same(pairs, cur):
    keep = pairs[:, 0] != pairs[:, 1]
    return pairs[keep], cur[keep]


@pytest.mark.parametrize("nk,nl,seed", MAPS)
def test_checker_equals_host_stage_after_every_pair(_built, nk, nl, seed):
    from ov2slam_amd import host_map
    m, d = the_map(nk, nl, seed)
    pairs, _ = without_same(*full_list(nk, nl, seed)[:2])
    hm = host_map.FilterMap(m)
    M = R.build(d)

    def same():
        _, lms, obs = hm.export()
        return (set(obs) == set(M["row"]) and set(lms) == set(M["lms"])
                and all(bool(s & R.LM_3D) == bool(M["tables"]["lm_state"][l] & R.LM_3D) for l, (_, s) in lms.items()))
    assert same(), "the two maps differ before the first pair"
    for i, (p, n) in enumerate(pairs.tolist()):
        host_merge(hm, p, n)
        R.merge_pair(M, p, n)
        assert same(), (i, p, n)
