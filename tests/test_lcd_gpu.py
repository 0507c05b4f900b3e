"""The loop detector's device word table and exact search (ov2_lcd_table_*, ov2_lcd_search2_batch) on the GPU against
tests/lcd_ref.py: exact equality of slot and distance for every split count, table sizes around the LDS tile, slots beyond
65 536, ties, dead slots, compaction, batches against single calls, the device-resident form, untouched output rows and
every refusal."""
import ctypes as C

import numpy as np
import pytest

import lcd_ref as R

pytestmark = pytest.mark.gpu

SPLITS = [0, 1, 2, 3, 7]
vp = C.c_void_p


@pytest.fixture(scope="module")
def L():
    from ov2slam_amd import lcd
    return lcd


@pytest.fixture()
def sctx(ctx, L):
    yield ctx
    L.set_splits(ctx, 0)


def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(row, *bits):
    r = row.copy()
    for bit in bits:
        r[bit // 8] ^= np.uint8(1 << (bit % 8))
    return r


def table_of(ctx, L, rows, dead=()):
    t = L.Table(ctx)
    if len(rows):
        assert t.append(rows) == 0
    if len(dead):
        t.kill(dead)
    return t


def check(got, queries, rows, dead=None, what=""):
    for b, ((gi, gd), q, r) in enumerate(zip(got, queries, rows)):
        ri, rd = R.search2(q, r, None if dead is None else dead[b])
        assert np.array_equal(gd, rd), f"{what} pair {b}: distances differ at rows {np.flatnonzero((gd != rd).any(1))[:8]}"
        assert np.array_equal(gi, ri), f"{what} pair {b}: slots differ at rows {np.flatnonzero((gi != ri).any(1))[:8]}"


def test_sizes_every_split(sctx, L):
    """every table size of the list against every query count, as one batch per split setting"""
    T = L.TILE
    rng = np.random.default_rng(1)
    sizes = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    n_query = [1, 63, 64, 65, 257]
    rows = {n: rand_rows(rng, n) for n in sizes}
    tabs = {n: table_of(sctx, L, rows[n]) for n in sizes}
    qs, ts, rs = [], [], []
    for nq in n_query:
        for n in sizes:
            qs.append(rand_rows(rng, nq)); ts.append(tabs[n]); rs.append(rows[n])
    ref = [R.search2(q, r) for q, r in zip(qs, rs)]
    for splits in SPLITS:
        L.set_splits(sctx, splits)
        got = L.search2_batch(sctx, ts, qs)
        for b, ((gi, gd), (ri, rd)) in enumerate(zip(got, ref)):
            assert np.array_equal(gd, rd) and np.array_equal(gi, ri), f"splits {splits}: {len(qs[b])} queries x {len(rs[b])} words differs"


def test_slots_beyond_65536(sctx, L):
    """66 000 rows; nearest and second nearest of some queries planted at slots >= 65 536 (beyond the matcher's key), on either
    side of a split boundary: 65 536 itself is one of the automatic choice (whole tiles), 65 538 and 65 604 of 1000 splits
    (66 rows each), and one pair straddles the last boundary of 7 splits"""
    rng = np.random.default_rng(2)
    n = 66000
    rows = rand_rows(rng, n)
    q = rand_rows(rng, 70)
    b7 = 6 * ((n + 6) // 7)
    plant = [(65537, 65538), (65999, 65550), (65535, 65536), (b7 - 1, 65540), (65700, 3), (65604, 65603), (b7, b7 - 2)]
    assert 66 * 993 == 65538 and 66 * 994 == 65604 and (n + 999) // 1000 == 66 and 65536 % L.TILE == 0
    for k, (a, b) in enumerate(plant):
        rows[a] = flipped(q[k], 3)               # distance 1
        rows[b] = flipped(q[k], 3, 77, 140)      # distance 3
    t = table_of(sctx, L, rows)
    ri, rd = R.search2(q, rows)
    for k, (a, b) in enumerate(plant):
        assert (ri[k, 0], ri[k, 1], rd[k, 0], rd[k, 1]) == (a, b, 1, 3)
    for splits in SPLITS + [1000]:
        L.set_splits(sctx, splits)
        (gi, gd), = L.search2_batch(sctx, [t], [q])
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd), f"splits {splits}"


def test_ties_go_to_the_lower_slot(sctx, L):
    T = L.TILE
    rng = np.random.default_rng(3)
    rows = rand_rows(rng, 2 * T + 40)
    rows[T + 17] = rows[5]                        # the same row in three tiles (and, with 2, 3, 7 splits, in different splits)
    rows[2 * T + 3] = rows[5]
    q = rand_rows(rng, 8)
    q[0] = rows[5]                                # a query equal to a row: distance 0 three times
    q[1] = flipped(rows[5], 9, 200)               # distance 2 to all three copies
    for s in (700, 30, 2 * T + 20):               # second neighbour tied three ways behind a unique nearest
        rows[s] = flipped(q[2], 1, 2, 3, 4)
    rows[400] = flipped(q[2], 250)
    rows[8], rows[9] = flipped(q[3], 7), flipped(q[3], 8)   # neighbours in one quad's rows
    t = table_of(sctx, L, rows)
    ri, rd = R.search2(q, rows)
    assert ri[0].tolist() == [5, T + 17] and rd[0].tolist() == [0, 0]
    assert ri[1].tolist() == [5, T + 17] and rd[1].tolist() == [2, 2]
    assert ri[2].tolist() == [400, 30] and rd[2].tolist() == [1, 4]
    assert ri[3].tolist() == [8, 9] and rd[3].tolist() == [1, 1]
    for splits in SPLITS:
        L.set_splits(sctx, splits)
        (gi, gd), = L.search2_batch(sctx, [t], [q])
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd), f"splits {splits}"


def test_dead_slots(sctx, L):
    rng = np.random.default_rng(4)
    rows = rand_rows(rng, 1300)
    q = rand_rows(rng, 66)
    rows[900], rows[17] = flipped(q[0], 5), flipped(q[0], 5, 6)
    t = table_of(sctx, L, rows)
    dead = np.zeros(len(rows), bool)
    (gi, gd), = L.search2_batch(sctx, [t], [q])
    assert gi[0].tolist() == [900, 17]
    t.kill([900]); dead[900] = True               # the planted nearest row killed
    assert t.count() == (1300, 1299, 0)
    for splits in SPLITS:
        L.set_splits(sctx, splits)
        got = L.search2_batch(sctx, [t], [q])
        check(got, [q], [rows], [dead], f"splits {splits}")
        assert got[0][0][0, 0] == 17
    L.set_splits(sctx, 0)
    t.kill([900])                                 # again: nothing changes
    assert t.count() == (1300, 1299, 0)
    # exactly one live row, then none (the table compacts itself on the way: slots <= 2 live + appended)
    t2 = table_of(sctx, L, rows[:70])
    t2.kill(np.delete(np.arange(70), 33))
    slots, live, comps = t2.count()
    assert live == 1 and slots <= 2 * live + 70
    ids, dd = t2.ids()
    (gi, gd), = L.search2_batch(sctx, [t2], [q])
    assert (gi[:, 1] == -1).all() and (gd[:, 1] == -1).all()
    assert (ids[gi[:, 0]] == 33).all() and np.array_equal(gd[:, 0], R.search2(q, rows[33:34])[1][:, 0])
    t2.kill([int(np.flatnonzero(ids == 33)[0])])
    assert t2.count()[1] == 0
    (gi, gd), = L.search2_batch(sctx, [t2], [q])
    assert (gi == -1).all() and (gd == -1).all()


def test_kill_compact_append(sctx, L):
    """slots are remapped as the ids array says, live rows keep their order, appended rows get new word ids"""
    rng = np.random.default_rng(5)
    rows = rand_rows(rng, 1100)
    q = rand_rows(rng, 40)
    t = table_of(sctx, L, rows)
    kill = np.unique(np.concatenate([rng.integers(0, 1100, 60), np.arange(1080, 1100), [0, 511, 512]]))
    t.kill(kill)
    assert t.count() == (1100, 1100 - len(kill), 0)
    t.compact()
    slots, live, comps = t.count()
    assert (slots, live, comps) == (1100 - len(kill), 1100 - len(kill), 1)
    ids, dd = t.ids()
    keep = np.setdiff1d(np.arange(1100), kill)
    assert np.array_equal(ids, keep) and not dd.any()
    more = rand_rows(rng, 77)
    more[5] = flipped(q[1], 1)
    assert t.append(more) == live
    ids, dd = t.ids()
    assert np.array_equal(ids, np.concatenate([keep, 1100 + np.arange(77)]))
    now = np.concatenate([rows[keep], more])
    for splits in (0, 3):
        L.set_splits(sctx, splits)
        got = L.search2_batch(sctx, [t], [q])
        check(got, [q], [now], None, f"splits {splits}")
    assert ids[got[0][0][1, 0]] == 1105
    t.compact()                                   # nothing dead: not a compaction
    assert t.count() == (len(now), len(now), 1)


def test_slots_live_bound_over_a_long_sequence(sctx, L):
    """slots <= 2 live + rows appended since the last compaction, after every step; the search agrees with a host model"""
    rng = np.random.default_rng(6)
    t = L.Table(sctx)
    model_ids, model_rows, next_id, appended, comps = [], {}, 0, 0, 0
    for step in range(60):
        new = rand_rows(rng, int(rng.integers(20, 150)))
        t.append(new)
        for r in new:
            model_ids.append(next_id); model_rows[next_id] = r; next_id += 1
        appended += len(new)
        ids, dd = t.ids()
        live_slots = np.flatnonzero(~dd)
        # the reference's pattern (recent words) on even steps, anywhere on odd ones
        pool = live_slots[-120:] if step % 2 == 0 else live_slots
        many = len(pool) * 7 // 10 if step % 10 == 9 else int(rng.integers(0, 110))   # now and then most of the table
        k = rng.choice(pool, size=min(len(pool), many), replace=False)
        t.kill(k)
        for w in ids[k]:
            model_ids.remove(int(w)); del model_rows[int(w)]
        slots, live, c = t.count()
        if c != comps:
            comps, appended = c, 0
        assert live == len(model_ids) and slots <= 2 * live + appended, (step, slots, live, appended)
        ids, dd = t.ids()
        assert np.array_equal(ids[~dd], model_ids)
    assert comps >= 3 and len(model_ids) > 100
    q = rand_rows(rng, 65)
    (gi, gd), = L.search2_batch(sctx, [t], [q])
    ri, rd = R.search2(q, np.stack([model_rows[w] for w in model_ids]))
    assert np.array_equal(gd, rd) and np.array_equal(ids[gi], np.asarray(model_ids)[ri])


def test_batch_against_single_calls_and_dev_form(sctx, L):
    rng = np.random.default_rng(7)
    sizes = [300, 0, 1, 5000, 64, 513, 2, 1025, 700]
    rows = [rand_rows(rng, n) for n in sizes]
    dead = [np.zeros(n, bool) for n in sizes]
    tabs = [table_of(sctx, L, r) for r in rows]
    tabs[3].kill(np.arange(100, 4000, 7)); dead[3][np.arange(100, 4000, 7)] = True
    qs = [rand_rows(rng, n) for n in (50, 3, 64, 129, 0, 65, 1, 200, 10)]
    batch = L.search2_batch(sctx, tabs, qs)
    check(batch, qs, rows, dead, "B = 9")
    for b in range(9):
        (gi, gd), = L.search2_batch(sctx, [tabs[b]], [qs[b]])
        assert np.array_equal(gi, batch[b][0]) and np.array_equal(gd, batch[b][1]), f"B = 1 call of pair {b}"
    flat_i, flat_d = np.concatenate([b[0] for b in batch]), np.concatenate([b[1] for b in batch])
    for splits in (0, 2):
        L.set_splits(sctx, splits)
        di, dd = L.search2_batch_dev(sctx, tabs, qs, fill=-7, extra_rows=5)
        assert np.array_equal(di[:-5], flat_i) and np.array_equal(dd[:-5], flat_d)
        assert (di[-5:] == -7).all() and (dd[-5:] == -7).all()   # rows behind the call's stay untouched


def test_empty_calls_write_nothing(sctx, L):
    rng = np.random.default_rng(8)
    t = table_of(sctx, L, rand_rows(rng, 10))
    before = L.search_calls(sctx)
    assert L.search2_batch(sctx, [], []) == []
    (gi, gd), = L.search2_batch(sctx, [t], [np.zeros((0, 32), np.uint8)])
    assert gi.shape == (0, 2)
    di, dd = L.search2_batch_dev(sctx, [t, t], [np.zeros((0, 32), np.uint8)] * 2, extra_rows=4)
    assert (di == -7).all() and (dd == -7).all()
    assert L.search_calls(sctx) == before


def test_refusals(sctx, L):
    lib, h = sctx.lib, sctx.h
    rng = np.random.default_rng(9)
    t = table_of(sctx, L, rand_rows(rng, 10))
    q = rand_rows(rng, 4)
    idx, dist = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.int32)
    hs = (vp * 1)(t.h)
    n1, nneg = (C.c_int * 1)(4), (C.c_int * 1)(-1)
    P = lambda a: a.ctypes.data_as(vp)
    bad = lambda st: st == -1   # OV2_ERR_INVALID
    assert bad(lib.ov2_lcd_set_splits(h, -1))
    assert bad(lib.ov2_lcd_set_splits(h, L.MAX_SPLITS + 1))
    assert bad(lib.ov2_lcd_search2_batch(h, -1, hs, n1, P(q), P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, None, n1, P(q), P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, None, P(q), P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, nneg, P(q), P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, n1, None, P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, n1, P(q), None, P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, n1, P(q), P(idx), None))
    assert bad(lib.ov2_lcd_search2_batch(h, 1, (vp * 1)(None), n1, P(q), P(idx), P(dist)))
    assert bad(lib.ov2_lcd_search2_batch(h, L.MAX_BATCH + 1, hs, n1, P(q), P(idx), P(dist)))
    nbig = (C.c_int * 1)(L.MAX_QUERY + 1)
    assert bad(lib.ov2_lcd_search2_batch(h, 1, hs, nbig, P(q), P(idx), P(dist)))
    d_q, d_i, d_d = sctx.to_device(np.zeros((5, 32), np.uint8)), sctx.to_device(idx), sctx.to_device(dist)
    assert bad(lib.ov2_lcd_search2_batch_dev(h, 1, hs, n1, vp(d_q.ptr.value + 8), d_i.ptr, d_d.ptr))   # misaligned
    assert b"aligned" in lib.ov2_last_error(h)
    out = vp()
    assert bad(lib.ov2_lcd_search2_batch_dev(h, 1, hs, n1, None, d_i.ptr, d_d.ptr))
    assert bad(lib.ov2_lcd_table_create(h, -1, C.byref(out))) and not out.value
    assert bad(lib.ov2_lcd_table_create(h, L.MAX_WORDS + 1, C.byref(out))) and not out.value   # on the count alone
    assert bad(lib.ov2_lcd_table_create(h, 16, None))
    first = C.c_int()
    assert bad(lib.ov2_lcd_table_append(h, t.h, -1, P(q), C.byref(first)))
    assert bad(lib.ov2_lcd_table_append(h, t.h, 4, None, C.byref(first)))
    assert bad(lib.ov2_lcd_table_append(h, t.h, L.MAX_WORDS, P(q), C.byref(first)))            # 10 + MAX_WORDS live words
    assert bad(lib.ov2_lcd_table_append(h, None, 4, P(q), C.byref(first)))
    s = np.array([3, 10], np.int32)
    assert bad(lib.ov2_lcd_table_kill(h, t.h, 2, P(s))) and t.count() == (10, 10, 0)           # slot 10 of 10: nothing marked
    assert bad(lib.ov2_lcd_table_kill(h, t.h, -1, P(s)))
    assert bad(lib.ov2_lcd_table_kill(h, t.h, 2, None))
    assert bad(lib.ov2_lcd_table_compact(h, None))
    assert lib.ov2_lcd_set_splits(h, 0) == 0
    (gi, gd), = L.search2_batch(sctx, [t], [q])   # and the table still serves
    ri, rd = R.search2(q, rand_rows(np.random.default_rng(9), 10))
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


# ---- the host detector on the device word table ----------------------------------------------------------------------------------

SMALL = dict(p=5, island_size=4, nframes_after_lc=3)


@pytest.fixture(scope="module")
def streams():
    import test_lcd_ref_cpu as T
    out = {}
    for name, (st, _) in T.make_streams().items():
        det = R.LCDetector(R.Params(**SMALL))
        run, kf_of = R.run_stream(det, st)
        out[name] = (st, run, det.trace)
    return out


def test_detector_on_the_device_equals_host_and_checker(sctx, L, streams):
    """every synth_lcd stream: statuses, train ids, kept matches, added / purged word ids and island limits equal, scores to
    1e-12 relative; the device table's live count is the host index's word count after every image"""
    from test_lcd_ref_cpu import assert_trace_equal
    for name, (st, run, trace) in streams.items():
        dd, hd = L.Detector(sctx, **SMALL), L.Detector(None, **SMALL)
        for (kf, img, status, train), t in zip(run, trace):
            got = dd.process(img, st[kf])
            assert got == (status, train) and hd.process(img, st[kf]) == got, (name, kf)
            dt = dd.trace()
            assert_trace_equal(dt, t, (name, kf))
            assert_trace_equal(dt, hd.trace(), (name, kf, "host"))
            c = dd.counts()
            assert c["dev_live"] == c["words"] == t["nwords"] and c["dev_slots"] <= 2 * c["dev_live"] + len(t["added"]), (name, kf)
        assert c["words"] > 100


def test_detector_survives_compaction_of_its_table(sctx, L):
    """purge off and on with images that share nothing: with purge on every word dies two images later, the table compacts
    under the detector again and again, and the device detector still equals the host one"""
    rng = np.random.default_rng(21)
    P = dict(p=1, island_size=4, nframes_after_lc=0)   # the gate is always open: every image asks
    dd, hd = L.Detector(sctx, **P), L.Detector(None, **P)
    imgs = [rand_rows(rng, 40) for _ in range(12)]
    imgs[7] = np.stack([flipped(r, 3, 99) for r in imgs[6]])       # image 7 repeats image 6: those words survive
    imgs[11] = np.stack([flipped(r, 5) for r in imgs[6][:20]])     # and image 11 finds them again
    for i, d in enumerate(imgs):
        got = dd.process(i, d)
        assert got == hd.process(i, d), i
        dt, ht = dd.trace(), hd.trace()
        assert dt["matches"] == ht["matches"] and dt["added"] == ht["added"] and dt["purged"] == ht["purged"] and dt["islands"] == ht["islands"]
        c = dd.counts()
        assert c["dev_live"] == c["words"] == hd.counts()["words"]
    assert c["dev_compactions"] >= 2 and len(dt["matches"]) == 20


def test_process_batch_equals_single_runs(sctx, L, streams):
    """5 detectors at different positions of different streams, stepped together: the same results as 5 single runs (the
    checker's), and at most two search calls per step whatever the number of detectors"""
    names = list(streams)
    lanes = [(names[k % 3], 7 * k) for k in range(5)]              # (stream, first step): detectors start 7 steps apart
    dets = [L.Detector(sctx, **SMALL) for _ in lanes]
    most = 0
    for step in range(40 + 7 * 4):
        act = [k for k, (nm, s0) in enumerate(lanes) if 0 <= step - s0 < len(streams[nm][1])]
        if not act:
            continue
        rows = [streams[lanes[k][0]][1][step - lanes[k][1]] for k in act]        # (kf, img, status, train) of the checker
        before = L.search_calls(sctx)
        got = L.process_batch([dets[k] for k in act], [r[1] for r in rows], [streams[lanes[k][0]][0][r[0]] for k, r in zip(act, rows)])
        most = max(most, L.search_calls(sctx) - before)
        assert got == [(r[2], r[3]) for r in rows], step
        for k, r in zip(act, rows):
            t = streams[lanes[k][0]][2][step - lanes[k][1]]
            dt = dets[k].trace()
            assert dt["matches"] == t["matches"] and dt["added"] == t["added"] and dt["purged"] == t["purged"], (step, k)
    assert most == 2


# ---- LoopCloser::newKeyframe on the revisit scene of synth_loop ---------------------------------------------------------------------

LC_PARAMS = dict(p=2, island_size=4, nframes_after_lc=0, purge_descriptors=False)


def revisit_map():
    """synth_loop's scene (keyframe 40 revisits keyframe 2 under other lmids) plus keyframe 1, whose two map points have no
    descriptor: the detector must skip it, and it is the closest older keyframe once keyframe 2 is gone"""
    from ov2slam_amd import host_map, synth_loop
    s = synth_loop.make_scene()
    s["kfids"] = [1] + list(s["kfids"])
    s["poses"][1] = np.array([0.05, 0, 0, 0, 0, 0, 1.0])
    s["kps"][1] = dict(lmid=np.array([90001, 90002], np.int32), uv=np.array([[50, 50], [80, 90]], np.float32), kp3d=np.zeros(2, np.uint8))
    return s, host_map.LoopMap(s)


@pytest.mark.parametrize("forget", [None, 2])
def test_new_keyframe_proposes_the_planted_pair(sctx, L, forget):
    from ov2slam_amd import host_map
    s, m = revisit_map()
    lc = L.LoopCloser(sctx, m, **LC_PARAMS)
    det = R.LCDetector(R.Params(**LC_PARAMS))
    try:
        img = 0
        for k in [k for k in s["kfids"] if k <= 40]:
            if k == 40 and forget is not None:
                host_map.lib().ov2h_map_forget_keyframe(m.h, forget)        # the planted keyframe leaves the map before the revisit
            rows = [s["desc"][l] for l in m.keypoint_order(k) if l in s["desc"] and l not in s["forget_lm"]]
            r = lc.new_keyframe(k, 77 + k)
            if not rows:
                assert k == 1 and r["skipped"] == 1 and r["image_id"] == -1 and r["stats"]["pairs"] == 0
                continue
            status, train = det.process(img, np.stack(rows))
            assert (r["skipped"], r["image_id"], r["status"]) == (0, img, status), k      # a skipped keyframe took no image id
            if status == R.LC_DETECTED:
                assert r["train_id"] == train and r["stats"]["pairs"] == 1, k             # the pair reached processLoopCandidates
            else:
                assert r["cand_kfid"] == -1 and r["stats"]["pairs"] == 0, k
            img += 1
        # keyframe 40: the checker finds image 0 = keyframe 2, the planted one
        assert (status, train) == (R.LC_DETECTED, 0) and lc.L is not None
        if forget is None:
            assert r["cand_kfid"] == 2 and r["lckfid"] == 2 and r["stats"]["knn_calls"] == 1   # the pair "clean" reaches the matcher
        else:
            assert r["cand_kfid"] == 1 and r["lckfid"] == 1   # the closest older keyframe still in the map
    finally:
        lc.close()
        m.close()
