"""Loop-candidate matching without a GPU: the matcher's checker (tests/knn_ref.py) against an independent formulation, the
acceptance rule of LoopCloser::knnMatching at its edges, removeOutliers with its wrap-around, the promises of the scene
generator (ov2slam_amd/synth_loop.py) asserted on the checker alone (tests/loop_ref.py), and the pair assembly of the C++
host mirror (ov2::LoopCloser::assembleKnn through the C API) against the checker's."""
import numpy as np
import pytest

from ov2slam_amd import synth_loop
import knn_ref as KR
import loop_ref as LR

NRANSAC, ERRTH, SEED = 10, 3.0, 1234


def slow_knn2(query, train):
    """Python integers, bin(x).count("1"), and a scan that replaces a kept neighbour only on a strictly smaller distance"""
    Q = [int.from_bytes(bytes(r), "little") for r in np.asarray(query, np.uint8).reshape(-1, 32)]
    T = [int.from_bytes(bytes(r), "little") for r in np.asarray(train, np.uint8).reshape(-1, 32)]
    idx, dist = [], []
    for q in Q:
        best = [(-1, -1), (-1, -1)]   # (dist, idx), nearest first
        for j, t in enumerate(T):
            d = bin(q ^ t).count("1")
            if best[0][1] < 0 or d < best[0][0]:
                best = [(d, j), best[0]]
            elif best[1][1] < 0 or d < best[1][0]:
                best[1] = (d, j)
        idx.append([best[0][1], best[1][1]])
        dist.append([best[0][0], best[1][0]])
    return np.array(idx, np.int32).reshape(-1, 2), np.array(dist, np.int32).reshape(-1, 2)


@pytest.mark.parametrize("nq,nt", [(7, 0), (7, 1), (7, 2), (9, 3), (33, 70), (5, 300)])
def test_knn_ref_against_python_integers(nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    q, t = rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    if nt >= 8:      # ties: copies of one row far apart, a query equal to a row, rows equally far from a query
        t[nt - 1] = t[0]
        q[0] = t[0]
        q[1] = synth_loop.flip(t[0], [5, 77])
        t[nt // 2] = synth_loop.flip(q[2], [1, 2, 3])
        t[1] = synth_loop.flip(q[2], [100, 200, 250])
    i0, d0 = KR.knn2(q, t)
    i1, d1 = slow_knn2(q, t)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    if nt >= 8:
        assert i0[0].tolist() == [0, nt - 1] and d0[0].tolist() == [0, 0] and d0[1].tolist() == [2, 2]
        assert sorted(i0[2].tolist()) == [1, nt // 2] and i0[2, 0] < i0[2, 1] and d0[2].tolist() == [3, 3]


def test_knn_ref_all_rows_equal():
    t = np.tile(np.arange(32, dtype=np.uint8), (40, 1))
    i, d = KR.knn2(np.zeros((3, 32), np.uint8), t)
    assert (i == [0, 1]).all() and (d[:, 0] == d[:, 1]).all()


def test_acceptance_rule_at_every_edge():
    """d0 <= maxdist && d0 <= d1 * 0.85 with the product in double: every listed pair sits exactly on the edge and passes,
    one more bit in d0 or one less in d1 fails"""
    for d0, d1 in synth_loop.RATIO_EDGES:
        assert d1 * 0.85 == d0, "the double product is exact at the listed pairs"
        assert LR.accept(d0, d1) and LR.accept(d0 - 1, d1) and LR.accept(d0, d1 + 1)
        assert not LR.accept(d0 + 1, d1) and not LR.accept(d0, d1 - 1)
    assert LR.MAXDIST == 128
    assert LR.accept(127, 254) and LR.accept(128, 255) and not LR.accept(129, 256)
    assert not LR.accept(128, 150) and LR.accept(128, 151)          # 150 * 0.85 = 127.5
    assert LR.accept(0, 0) and not LR.accept(1, 1) and not LR.accept(6, 7) and LR.accept(5, 6) and not LR.accept(5, 5)
    assert LR.accept(200, -1) and LR.accept(0, -1)                   # fewer than two neighbours: accepted untested


def test_remove_outliers_wrap_around():
    pairs = [(i, 100 + i) for i in range(8)]
    assert LR.remove_outliers(pairs, []) == pairs
    assert LR.remove_outliers(pairs, [2, 5]) == [pairs[i] for i in (0, 1, 3, 4, 6, 7)]
    assert LR.remove_outliers(pairs, [7]) == pairs[:7]
    # after the last outlier j wraps to entry 0, which is -1 by then: nothing else goes, even a repeated index
    assert LR.remove_outliers(pairs, [0]) == pairs[1:]
    # indices that do not ascend: 5 is waited for first, 2 is never reached
    assert LR.remove_outliers(pairs, [5, 2]) == [pairs[i] for i in (0, 1, 2, 3, 4, 6, 7)]


# ---- the scene and the C++ host mirror ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """the scene, the mirror's map of it, the mirror's keypoint order, the checker's result per pair (computed once)"""
    import __graft_entry__ as g
    g.build()
    from ov2slam_amd import host_map
    s = synth_loop.make_scene(0)
    hm = host_map.LoopMap(s)
    order = hm.order()
    S = LR.Scene(s)
    ref = {name: S.process(a, b, SEED, order, NRANSAC, ERRTH) for name, (a, b) in s["pairs"].items()}
    return s, hm, order, S, ref


def test_scene_promises(world):
    s, _, order, S, ref = world
    eff = s["effects"]
    assert s["pairs"]["clean"][0] - s["pairs"]["clean"][1] > 30
    # every gate branch is taken by some pair
    assert ref["covisible"]["branch"] == LR.COVISIBLE and ref["covisible"]["knn"] == []
    assert ref["cov30"]["branch"] == LR.FEW_MATCHES and ref["few"]["branch"] == LR.FEW_MATCHES
    assert 0 < len(ref["few"]["knn"]) < 15
    assert ref["nogeom"]["branch"] == LR.FILTER_FAILED and len(ref["nogeom"]["knn"]) >= 15 and ref["nogeom"]["status"] == 0
    assert ref["walkdown"]["lckfid"] == 7 and ref["walkdown"]["knn"] == ref["nogeom"]["knn"]
    assert ref["empty"]["branch"] == LR.FEW_MATCHES and ref["empty"]["sets"][2] == [] and ref["empty"]["knn"] == []
    c = ref["clean"]
    assert c["branch"] == LR.PASSED and c["status"] == 2 and len(c["out"]) >= 30
    ident, query, train = c["sets"]
    knn, out = set(c["knn"]), set(c["out"])
    # the smaller effects, in the stated numbers, and what becomes of each
    assert len(eff["true"]) >= 60 and s["true_pairs"] <= knn
    assert len(eff["wrong"]) >= 5 and s["wrong_pairs"] <= knn and not (s["wrong_pairs"] & out)     # accepted, then removed
    assert len(s["true_pairs"] & out) >= 0.9 * len(s["true_pairs"]) and c["n_outliers"] >= len(s["wrong_pairs"])
    acc_q = {a for a, b in knn if a != b}
    assert len(eff["distractor_query"]) >= 5 and set(eff["distractor_query"]) <= set(query) and not (set(eff["distractor_query"]) & acc_q)
    assert len(eff["distractor_train"]) >= 5 and set(eff["distractor_train"]) <= set(train)
    assert len(eff["ambiguous"]) >= 5 and set(eff["ambiguous"]) <= set(query) and not (set(eff["ambiguous"]) & acc_q)
    assert len(eff["shared3d"]) >= 5 and sorted(ident) == sorted(eff["shared3d"]) and {(l, l) for l in ident} <= knn
    assert len(eff["shared2d"]) >= 5 and set(eff["shared2d"]) <= set(query) and not (set(eff["shared2d"]) & set(train))
    assert len(eff["no_desc"]) >= 5 and not (set(eff["no_desc"]) & (set(query) | set(train)))
    assert len(eff["absent"]) >= 5 and not (set(eff["absent"]) & (set(query) | set(train))) and set(eff["absent"]) == set(s["forget_lm"])
    # ties: both train rows at the same distance, far apart in the train set; the exact copies are accepted with the lower row
    idx, dist = KR.knn2(np.stack([S.desc[l] for l in query]), np.stack([S.desc[l] for l in train]))
    far = 0
    for l in eff["tie_far"] + eff["tie_exact"]:
        q = query.index(l)
        assert dist[q, 0] == dist[q, 1] == (5 if l in eff["tie_far"] else 0) and idx[q, 0] < idx[q, 1]
        far += idx[q, 1] - idx[q, 0] > 16
        assert (l in acc_q) == (l in eff["tie_exact"])
        if l in eff["tie_exact"]:
            assert (l, train[idx[q, 0]]) in knn
    assert len(eff["tie_far"]) >= 3 and len(eff["tie_exact"]) >= 3 and far >= 4
    # the ratio edges and maxdist: the matcher sees exactly the distances the generator built, and the rule splits them
    for name, lst in (("edge_odd", s["ratio_edges"]), ("edge_even", s["ratio_edges"]), ("edge_max", s["maxdist_edges"])):
        r = ref[name]
        _, query, train = r["sets"]
        idx, dist = KR.knn2(np.stack([S.desc[l] for l in query]), np.stack([S.desc[l] for l in train]))
        acc = {a for a, _ in r["knn"]}
        mine = [e for e in lst if e["query"] in query]
        assert len(mine) == len(query)
        for e in mine:
            q = query.index(e["query"])
            assert dist[q].tolist() == [e["d0"], e["d1"]] and train[idx[q, 0]] == e["first"]
            assert (e["query"] in acc) == LR.accept(e["d0"], e["d1"])
    seen = {(e["d0"], e["d1"]) for e in s["ratio_edges"]}
    assert seen == set(synth_loop.ratio_edge_targets()) and len(seen) == 30
    assert {e["d0"] for e in s["maxdist_edges"]} == {127, 128, 129}
    assert sum(LR.accept(e["d0"], e["d1"]) for e in s["ratio_edges"]) == 18 and sum(LR.accept(e["d0"], e["d1"]) for e in s["maxdist_edges"]) == 2


def test_host_assembly_equals_checker(world):
    """ov2::LoopCloser::assembleKnn through the C API: identity pairs, query and train lmids in the mirror's own iteration
    order, and the descriptor rows the matcher would receive"""
    s, hm, order, S, ref = world
    for name, (a, b) in s["pairs"].items():
        if name == "walkdown":
            with pytest.raises(RuntimeError):
                hm.assemble(a, b)          # keyframe 9 is not in the map; the walk down is the driver's
            continue
        ident, query, train = S.assemble(a, b, order)
        hi, hq, ht, qd, td = hm.assemble(a, b)
        assert (hi, hq, ht) == (ident, query, train), name
        assert np.array_equal(qd, np.array([S.desc[l] for l in query], np.uint8).reshape(-1, 32)), name
        assert np.array_equal(td, np.array([S.desc[l] for l in train], np.uint8).reshape(-1, 32)), name
    assert len(ref["clean"]["sets"][1]) > 64 and len(ref["clean"]["sets"][2]) > 64


def test_host_rule_and_remove_outliers_equal_checker(world):
    from ov2slam_amd import host_map
    import ctypes as C
    L = host_map.lib()
    for d0 in range(0, 140):
        for d1 in list(range(max(d0 - 1, 0), min(d0 + 40, 257))) + [-1]:
            assert bool(L.ov2h_loop_accept(d0, d1)) == LR.accept(d0, d1), (d0, d1)
    pairs = [(i, 100 + i) for i in range(9)]
    for outl in ([2, 5], [8], [0], [0, 1, 2, 3], [5, 2], [3, 3]):
        a = np.array(pairs, np.int32)
        o = np.array(outl, np.int32)
        n = L.ov2h_loop_remove_outliers(len(pairs), a.ctypes.data_as(C.POINTER(C.c_int)), len(o), o.ctypes.data_as(C.POINTER(C.c_int)))
        assert [tuple(r) for r in a[:n].tolist()] == LR.remove_outliers(pairs, outl), outl


def test_python_limits_equal_the_header():
    import os
    import re
    from ov2slam_amd import knn
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ov2slam_hip.h")).read()
    val = {m.group(1): 1 << int(m.group(3)) if m.group(3) else int(m.group(2))
           for m in re.finditer(r"#define OV2_KNN_(\w+) (\(1 << (\d+)\)|\d+)", txt)}
    assert val == dict(MAX_TRAIN=knn.MAX_TRAIN, MAX_ROWS=knn.MAX_ROWS, MAX_BATCH=knn.MAX_BATCH, TILE=knn.TILE)
    assert knn.MAX_TRAIN == 1 << 16      # the row index shares a 32-bit key with the distance: (dist << 16) | idx
