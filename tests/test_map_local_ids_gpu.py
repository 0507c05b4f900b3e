"""Local-map selection on the map mirrors (ov2_map_enable_local_sets, ov2_map_set_local_set / ov2_map_get_local_set,
ov2_map_local_ids_batch, csrc/map.hip) against the numpy checker (tests/local_ids_ref.py, itself checked against the C++ host
stage by tests/test_local_ids_ref_cpu.py) on the cases of tests/local_ids_cases.py; the id pool through growth, squeeze and
table growth; the refusals; and match_local_from_mirror against the matcher fed the host stage's set.  Only integers come out:
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import local_ids_cases as LC
import local_ids_ref as R
from ov2slam_amd import device_map as DM, frontend, host_map, synth_match as SM

pytestmark = pytest.mark.gpu
INVALID = -1   # OV2_ERR_INVALID (include/ov2slam_hip.h)
SPAN = 1 << 20  # OV2_LOCAL_SET_LMID_SPAN
SEEDS = (1, 2, 3)
GATES = (SM.FMAXPROJERR, SM.FDISTRATIO)
NAMES = LC.NAMES
FIELDS = ("cov_kfid", "cov_score", "oldest_cov", "n_fresh", "swapped", "extended", "lmid")


@pytest.fixture(scope="module")
def cases():
    import __graft_entry__ as g
    g.build()
    return {c["name"]: c for c in LC.make_cases()}


def apply_edits(m, edits):
    for e in edits:
        if e[0] == "remove_obs":
            m.remove_obs([e[1]], [e[2]])
        elif e[0] == "remove_keyframe":
            m.remove_keyframe(e[1])
        elif e[0] == "remove_landmarks":
            m.remove_landmarks(e[1])
        else:
            raise ValueError(e[0])


def mirror(ctx, c, pool_hint=0, local=True, capacity=None):
    """the case's map through the public hooks: the scene, its landmark states, the stored sets (handed over in a shuffled
    order), then the edits"""
    s = c["scene"]
    m = DM.DeviceMap.from_scene(ctx, s, capacity=capacity)
    m.newkf = c["k"]
    t0 = LC.table_of(s)
    lmids = np.flatnonzero(t0["lm_state"]).astype(np.int32)
    m.set_landmarks(lmids, None, t0["lm_state"][lmids])
    if local:
        m.enable_local_sets(pool_hint)
        rng = np.random.default_rng(5)
        for kf, ids in c["sets"].items():
            m.set_local_set(kf, rng.permutation(ids))
    apply_edits(m, c["edits"])
    return m


def plain(rec):
    return {k: (np.asarray(rec[k]).tolist() if k in ("cov_kfid", "cov_score", "lmid") else int(rec[k])) for k in FIELDS}


def want_of(c, sets=None):
    return plain(LC.expected(c, sets))


def live_set(d):
    kf, lm = R.live_rows(d)
    return set(zip(kf.tolist(), lm.tolist()))


def close(maps):
    for m in maps:
        m.close()


# ---- 1. every case against the checker ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_checker(ctx, cases, name):
    c = cases[name]
    m = mirror(ctx, c)
    d = m.download()
    assert live_set(d) == live_set(c["table"])                      # the mirror holds the table the checker works on
    alive = np.flatnonzero(c["table"]["lm_state"])
    assert np.array_equal(d["lm_state"][alive], c["table"]["lm_state"][alive])
    rec = DM.local_ids_batch(ctx, [m], [c["k"]], c["extend"], c["nmax"])[0]
    want = want_of(c)
    assert plain(rec) == want
    assert (rec["swapped"], rec["extended"]) == (c["swapped"], c["extended"])
    # the stored set of k is the reported list, on the host side and in the pool
    assert m.get_local_set(c["k"]).tolist() == want["lmid"]
    assert DM.fetch_dev(ctx, rec["d_lmid"], len(want["lmid"]), np.int32).tolist() == want["lmid"]
    assert DM.fetch_dev(ctx, rec["d_n_local"], 1, np.int32).tolist() == [len(want["lmid"])]
    few, n = m.get_local_set(c["k"], cap=3)
    assert n == len(want["lmid"]) and few.tolist() == want["lmid"][:3]     # n is reported even when cap is too small
    # every other live keyframe keeps what it had
    for kf in c["scene"]["kfids"]:
        if kf != c["k"] and c["table"]["kf_state"][kf]:
            assert m.get_local_set(kf).tolist() == c["sets"].get(kf, [])
    assert np.array_equal(m.download()["lm_state"], d["lm_state"]) and live_set(m.download()) == live_set(d)   # the tables are read only
    m.close()


# ---- 2. a batch is its single calls, in any order; the launch count does not follow B ----------------------------------------
def test_batch_equals_single_calls_and_launch_count(ctx, cases):
    cs = [cases[n] for n in ("extend_taken_after_union", "padded_ids", "empty_C")]      # three capacities, three branches
    assert len({(c["extend"], c["nmax"]) for c in cs}) == 1
    ext, nmax = cs[0]["extend"], cs[0]["nmax"]
    want = [want_of(c) for c in cs]
    ctx.kernel_timing(True)
    try:
        ctx.kernel_times()
        maps = [mirror(ctx, c) for c in cs]
        ctx.kernel_times()                                                    # the hooks' own kernels (edits) are not counted
        got = DM.local_ids_batch(ctx, maps, [c["k"] for c in cs], ext, nmax)
        n3 = sum(v[1] for v in ctx.kernel_times().values())
        assert [plain(r) for r in got] == want
        for b, c in enumerate(cs):
            one = mirror(ctx, c)
            ctx.kernel_times()
            r1 = DM.local_ids_batch(ctx, [one], [c["k"]], ext, nmax)[0]
            n1 = sum(v[1] for v in ctx.kernel_times().values())
            assert plain(r1) == want[b] and n1 == n3 == 9
            assert one.get_local_set(c["k"]).tolist() == maps[b].get_local_set(c["k"]).tolist() == want[b]["lmid"]
            one.close()
    finally:
        ctx.kernel_timing(False)
    order = [2, 0, 1]
    perm = [mirror(ctx, cs[b]) for b in order]
    got = DM.local_ids_batch(ctx, perm, [cs[b]["k"] for b in order], ext, nmax)
    assert [plain(r) for r in got] == [want[b] for b in order]
    close(maps + perm)


# ---- 3. a second keyframe reads what the first stored ---------------------------------------------------------------------
def test_two_keyframes_in_sequence(ctx, cases):
    c = cases["plain_swap"]
    k1 = want_of(c)["oldest_cov"]
    sets = {}
    r1 = R.local_ids(c["table"], sets, k1, False, 0)
    sets[k1] = r1["lmid"]
    r2 = R.local_ids(c["table"], sets, c["k"], True, LC.NMAX_BIG)
    assert r2["extended"] and r2["oldest_cov"] == k1 and set(r1["lmid"]) - set(r2["fresh"])      # the extension adds ids of its own
    m = mirror(ctx, c)
    g1 = DM.local_ids_batch(ctx, [m], [k1], False, 0)[0]
    g2 = DM.local_ids_batch(ctx, [m], [c["k"]], True, LC.NMAX_BIG)[0]
    assert plain(g1) == plain(r1) and plain(g2) == plain(r2)
    assert m.get_local_set(k1).tolist() == r1["lmid"] and m.get_local_set(c["k"]).tolist() == r2["lmid"]
    # a third call on the same keyframe meets its own set as `old`: the store rule decides on the stored count
    sets[c["k"]] = r2["lmid"]
    r3 = R.local_ids(c["table"], sets, c["k"], False, 0)
    assert plain(DM.local_ids_batch(ctx, [m], [c["k"]], False, 0)[0]) == plain(r3) and r3["swapped"] == int(2 * r3["n_fresh"] > len(r2["lmid"]))
    m.close()


# ---- 4. the pool: growth, squeeze, growth of the keyframe capacity ----------------------------------------------------------
def test_pool_growth_squeeze_and_table_growth(ctx, cases):
    c = cases["extend_taken"]
    m = mirror(ctx, c, pool_hint=8)
    p0 = m.local_pool()
    assert p0["capacity"] >= 8 and p0["squeezes"] == 0 and p0["used"] == p0["live"] == sum(len(v) for v in c["sets"].values())
    assert p0["capacity"] > 8                                        # the sets of the case did not fit the hint: it grew
    big = np.arange(20000, 22500, dtype=np.int32)
    spare = [kf for kf in c["scene"]["kfids"] if kf != c["k"] and kf not in c["sets"]][0]
    for r in range(3):                                               # a set replaced over and over leaves garbage behind
        m.set_local_set(spare, big[r:] if r < 2 else big[:40])
    p1 = m.local_pool()
    assert p1["squeezes"] == 0 and p1["used"] >= 4096 and 2 * p1["live"] < p1["used"]
    sets = dict(c["sets"])
    sets[spare] = big[:40].tolist()
    rec = DM.local_ids_batch(ctx, [m], [c["k"]], c["extend"], c["nmax"])[0]      # reserves first: the squeeze happens here
    p2 = m.local_pool()
    assert p2["squeezes"] == 1 and p2["used"] == p2["live"] == p1["live"] + len(rec["lmid"]) and p2["capacity"] >= p2["used"]
    want = want_of(c, sets)
    assert plain(rec) == want
    sets[c["k"]] = want["lmid"]
    for kf, ids in sets.items():
        assert m.get_local_set(kf).tolist() == sorted(ids)
    # the keyframe capacity grows: the per-keyframe columns travel, the pool stays
    cap_kf = len(m.download()["kf_state"])
    m.add_keyframe_px(cap_kf + 40, np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 2), np.float32))
    assert len(m.download()["kf_state"]) > cap_kf + 40
    for kf, ids in sets.items():
        assert m.get_local_set(kf).tolist() == sorted(ids)
    assert m.get_local_set(cap_kf + 40).tolist() == []
    rec = DM.local_ids_batch(ctx, [m], [c["k"]], c["extend"], c["nmax"])[0]
    assert plain(rec) == want_of(c, sets)
    m.close()


# ---- 5. a removed keyframe's set is unreadable ------------------------------------------------------------------------------
def test_removed_keyframe_set_is_refused(ctx, cases):
    c = cases["extend_taken"]
    m = mirror(ctx, c)
    kf = sorted(c["sets"])[0]
    live = m.local_pool()["live"]
    m.remove_keyframe(kf)
    n = C.c_int(-5)
    assert ctx.lib.ov2_map_get_local_set(m.h, kf, 0, None, C.byref(n)) == INVALID and n.value == -5
    ids = np.arange(3, dtype=np.int32)
    assert ctx.lib.ov2_map_set_local_set(m.h, kf, 3, ids.ctypes.data_as(C.c_void_p)) == INVALID
    assert m.local_pool()["live"] == live - len(c["sets"][kf])
    # the stage reads it as empty: what the checker gives without that keyframe and without its set
    t = LC.table_of(c["scene"], c["edits"] + [("remove_keyframe", kf)])
    sets = {k: v for k, v in c["sets"].items() if k != kf}
    want = plain(R.local_ids(t, sets, c["k"], c["extend"], c["nmax"]))
    assert plain(DM.local_ids_batch(ctx, [m], [c["k"]], c["extend"], c["nmax"])[0]) == want and kf not in want["cov_kfid"]
    m.close()


def test_set_local_set_refuses_duplicates_and_sorts(ctx, cases):
    c = cases["plain_swap"]
    m = mirror(ctx, c)
    before = m.local_pool()
    dup = np.array([7, 3, 7], np.int32)
    assert ctx.lib.ov2_map_set_local_set(m.h, 15, 3, dup.ctypes.data_as(C.c_void_p)) == INVALID
    neg = np.array([7, -3], np.int32)
    assert ctx.lib.ov2_map_set_local_set(m.h, 15, 2, neg.ctypes.data_as(C.c_void_p)) == INVALID
    cap_lm = len(m.download()["lm_state"])
    far = np.array([4, cap_lm + SPAN], np.int32)                     # one stray id must not grow the tables by gigabytes
    assert ctx.lib.ov2_map_set_local_set(m.h, 15, 2, far.ctypes.data_as(C.c_void_p)) == INVALID
    assert m.local_pool() == before and m.get_local_set(15).tolist() == [] and len(m.download()["lm_state"]) == cap_lm
    m.set_local_set(15, [9, 2, 700, 5])
    assert m.get_local_set(15).tolist() == [2, 5, 9, 700]
    m.set_local_set(15, [])
    assert m.get_local_set(15).tolist() == [] and m.local_pool()["live"] == before["live"]
    m.close()


def test_restore_forgets_the_set_of_a_keyframe_it_removes(ctx, cases):
    c = cases["extend_taken"]
    m = mirror(ctx, c)
    kept = sorted(c["sets"])[0]
    m.save_state()
    late = 40                                                        # enters after the save, without rows: the restore takes it out
    assert not c["table"]["kf_state"][late]
    m.add_keyframe_px(late, np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 2), np.float32))
    m.set_local_set(late, [3, 1, 2])
    m.set_local_set(kept, [8, 6])                                    # the sets are not saved state: this one stays as it is now
    live = m.local_pool()["live"]
    DM.restore_state_batch(ctx, [m])
    n = C.c_int()
    assert ctx.lib.ov2_map_get_local_set(m.h, late, 0, None, C.byref(n)) == INVALID
    assert m.local_pool()["live"] == live - 3 and m.get_local_set(kept).tolist() == [6, 8]
    m.add_keyframe_px(late, np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 2), np.float32))
    assert m.get_local_set(late).tolist() == []                      # the id comes back without the stale set
    m.close()


# ---- 6. refusals leave the maps untouched -------------------------------------------------------------------------------------
def test_refusals_leave_the_maps_untouched(ctx, cases):
    c = cases["extend_taken"]
    m, other, bare = mirror(ctx, c), mirror(ctx, c), mirror(ctx, c, local=False)
    ctx2 = frontend.Context(0)
    foreign = mirror(ctx2, c)
    L = ctx.lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(hs, kfs, out=True, nmax=10, ctx_=ctx):
        o = (DM.LocalIdsC * len(hs))() if out else None
        return L.ov2_map_local_ids_batch(ctx_.h, len(hs), (C.c_void_p * len(hs))(*hs), vp(np.array(kfs, np.int32)), 1, nmax, o)

    def snapshot(x):
        return (x.download()["lm_state"].tobytes(), live_set(x.download()), x.local_pool(), {k: x.get_local_set(k).tolist() for k in c["sets"]},
                x.get_local_set(c["k"]).tolist())
    s_m, s_o = snapshot(m), snapshot(other)
    k = c["k"]
    assert call([m.h, bare.h], [k, k]) == INVALID                    # a map without local sets
    assert call([m.h, foreign.h], [k, k]) == INVALID                 # a map of another context
    assert call([m.h, other.h, m.h], [k, k, k]) == INVALID           # listed twice
    assert call([m.h, other.h], [k, 25]) == INVALID                  # a keyframe that is not alive (25 never entered the map)
    assert call([m.h, other.h], [k, 100000]) == INVALID              # ... or lies outside the table
    assert call([m.h, other.h], [k, k], out=False) == INVALID        # out == NULL
    assert call([m.h, other.h], [k, k], nmax=-1) == INVALID
    assert L.ov2_map_local_ids_batch(ctx.h, -1, None, None, 0, 0, None) == INVALID
    assert snapshot(m) == s_m and snapshot(other) == s_o
    assert L.ov2_map_local_ids_batch(ctx.h, 0, None, None, 0, 0, None) == 0
    assert snapshot(m) == s_m
    n = C.c_int()
    assert L.ov2_map_get_local_set(bare.h, k, 0, None, C.byref(n)) == INVALID and L.ov2_map_local_pool(bare.h, None, None, None, None) == INVALID
    assert call([m.h, other.h], [k, k], nmax=LC.NMAX_BIG) == 0 and m.get_local_set(k).tolist() == want_of(c)["lmid"]   # and the maps still work
    close([m, other, bare, foreign])
    ctx2.close()


# ---- 7. a map without the local sets is what it was ---------------------------------------------------------------------------
def test_map_without_local_sets_behaves_as_before(ctx, cases):
    c = cases["plain_swap"]
    bare, twin = mirror(ctx, c, local=False), mirror(ctx, c)
    DM.local_ids_batch(ctx, [twin], [c["k"]], True, LC.NMAX_BIG)
    fresh = want_of(c)["lmid"]
    pairs = np.array([[fresh[0], fresh[1]], [fresh[2], fresh[3]]], np.int32)
    res = []
    for m in (bare, twin):
        v = DM.setup_batch(ctx, [m], newkf=[c["k"]], nmin_covscore=5, calib_l=SM.K4)[0]
        flat = DM.fetch_view(ctx, v, True)
        hdr, st = DM.merge_points_batch(ctx, [m], [pairs])
        res.append((flat, hdr, [s.tolist() for s in st], m.download()))
    (fa, ha, sa, da), (fb, hb, sb, db) = res
    assert not fa["aborted"] and len(fa["res_type"]) > 0 and sorted(fa) == sorted(fb)
    assert all(np.array_equal(fa[k], fb[k]) for k in fa) and ha == hb and sa == sb and ha[0]["n_merged"] >= 1
    assert DM.canonical_state(da) == DM.canonical_state(db)             # live entries: spare slots hold whatever the allocation held
    assert twin.get_local_set(c["k"]).tolist() == fresh               # a merge does not edit a stored set
    close([bare, twin])


# ---- 8. ids -> gather -> match on a mirror-only map ---------------------------------------------------------------------------
def grid_of(px_lists):
    nbw, nbh = int(np.ceil(SM.W / SM.CELL)), int(np.ceil(SM.H / SM.CELL))
    cells = [[] for _ in range(len(px_lists) * nbw * nbh)]
    for b, px in enumerate(px_lists):
        for i, p in enumerate(px):
            cells[b * nbw * nbh + int(np.floor(p[1] / SM.CELL)) * nbw + int(np.floor(p[0] / SM.CELL))].append(i)
    ptr = np.concatenate([[0], np.cumsum([len(cc) for cc in cells])]).astype(np.int32)
    return ptr, np.array([i for cc in cells for i in cc], np.int32)


@pytest.fixture(scope="module")
def match_jobs():
    """per seed: the case-shaped scene, and the local set of the new keyframe as the HOST stage builds it, sorted ascending"""
    import __graft_entry__ as g
    g.build()
    jobs = []
    for seed in SEEDS:
        s, gone = LC.base_scene(seed)
        c = dict(scene=s, k=LC.NEWKF, edits=gone, sets={}, table=LC.table_of(s, gone))
        hm = host_map.LoopMap(s)
        for l in gone[0][1]:
            hm.remove_landmark(l)
        hm.update_frame_covisibility(LC.NEWKF)
        assert hm.extend_local_map(LC.NEWKF, LC.NMAX_BIG)
        c["host_set"] = sorted(hm.local_ids(LC.NEWKF))
        hm.close()
        jobs.append(c)
    return jobs


@pytest.mark.parametrize("sel", [(0,), (0, 1, 2)])
def test_match_from_mirror_equals_match_on_the_host_set(ctx, match_jobs, sel):
    js = [match_jobs[i] for i in sel]
    kps = [j["scene"]["kps"][LC.NEWKF]["lmid"].tolist() for j in js]
    grids = grid_of([j["scene"]["kps"][LC.NEWKF]["uv"] for j in js])
    nb3d = [int(j["scene"]["kps"][LC.NEWKF]["kp3d"].sum()) for j in js]
    newkf = [LC.NEWKF] * len(js)
    ref_maps, maps = [mirror(ctx, j, local=False) for j in js], [mirror(ctx, j) for j in js]
    want = DM.match_local_batch(ctx, ref_maps, newkf, nb3d, kps, grids, [j["host_set"] for j in js], SM.CAMERA, fmaxprojerr=GATES[0],
                                fdistratio=GATES[1])
    got, ids = DM.match_local_from_mirror(ctx, maps, newkf, nb3d, kps, grids, SM.CAMERA, extend=True, nmax_local=LC.NMAX_BIG,
                                          fmaxprojerr=GATES[0], fdistratio=GATES[1])
    for (wl, wd), (gl, gd), r, j in zip(want, got, ids, js):
        assert r["lmid"].tolist() == j["host_set"] and len(j["host_set"]) > 100
        assert np.array_equal(wl, gl) and np.array_equal(wd, gd) and (gl >= 0).sum() > 20
    close(ref_maps + maps)
