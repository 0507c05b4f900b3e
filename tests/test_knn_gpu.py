"""ov2_knn2_hamming_batch on the GPU against tests/knn_ref.py: exact equality of idx and dist for every lane mapping, sizes
around the wave, the lane groups and the LDS tile, ties of every kind, batches against single calls, the device-resident
form, the slots the header leaves untouched, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import knn_ref as R

pytestmark = pytest.mark.gpu

LANES = [0, 1, 4, 16, 64]


@pytest.fixture(scope="module")
def K():
    from ov2slam_amd import knn
    return knn


@pytest.fixture()
def lanes_ctx(ctx):
    yield ctx
    ctx.set_knn_lanes(0)


def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(row, bit):
    r = row.copy()
    r[bit // 8] ^= np.uint8(1 << (bit % 8))
    return r


def assert_pairs_equal(got, queries, trains, what=""):
    for b, ((gi, gd), (ri, rd)) in enumerate(zip(got, R.knn2_batch(queries, trains))):
        assert np.array_equal(gd, rd), f"{what} pair {b}: distances differ at rows {np.flatnonzero((gd != rd).any(1))[:8]}"
        assert np.array_equal(gi, ri), f"{what} pair {b}: indices differ at rows {np.flatnonzero((gi != ri).any(1))[:8]}"


def test_sizes_every_lane_mapping(lanes_ctx, K):
    """every n_train of the list against every n_query, as one batch per lane mapping (a call per size pair would cost 55
    synchronisations per mapping for the same kernel paths)"""
    T = K.TILE
    rng = np.random.default_rng(1)
    n_train = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    n_query = [1, 63, 64, 65, 257]
    trains = {n: rand_rows(rng, n) for n in n_train}
    qs, ts = [], []
    for nq in n_query:
        for nt in n_train:
            qs.append(rand_rows(rng, nq))
            ts.append(trains[nt])
    ref = R.knn2_batch(qs, ts)
    for lanes in LANES:
        lanes_ctx.set_knn_lanes(lanes)
        got = K.knn2_hamming_batch(lanes_ctx, qs, ts)
        for b, ((gi, gd), (ri, rd)) in enumerate(zip(got, ref)):
            assert np.array_equal(gd, rd) and np.array_equal(gi, ri), f"lanes {lanes}: n_query {len(qs[b])} x n_train {len(ts[b])} differs"


def tie_cases(T):
    rng = np.random.default_rng(2)
    cases = {}
    # the same row in two different tiles: the earlier tile wins both slots in row order
    t = rand_rows(rng, 2 * T + 40)
    t[T + 17] = t[5]
    t[2 * T + 3] = t[5]
    q = rand_rows(rng, 9)
    q[0] = t[5]                      # distance 0, twice more at distance 0
    q[1] = t[5]; q[1, 3] ^= 0x11     # distance 2 to all three copies
    cases["copies in different tiles"] = (q, t)
    # the same row in different lanes' shares: rows r and r + 1 (lanes 4, 16, 64), r and r + 5, r and r + 37
    t = rand_rows(rng, 200)
    for a, b in ((10, 11), (20, 25), (40, 77), (130, 3)):
        t[b] = t[a]
    q = np.stack([t[10], t[20], t[40], t[130], flipped(t[11], 77)])
    cases["copies in different lanes' shares"] = (q, t)
    # a tie that straddles the last, partial tile
    t = rand_rows(rng, T + 3)
    t[T + 2] = t[T - 1]
    t[T + 1] = t[2]
    q = np.stack([t[T - 1], t[2], flipped(t[T + 2], 255)])
    cases["tie across the last partial tile"] = (q, t)
    # a query that is a train row, among unrelated rows
    t = rand_rows(rng, 70)
    cases["query equals a train row"] = (t[[69, 0, 33]].copy(), t)
    # all train rows equal: every query gets rows 0 and 1
    t = np.tile(rand_rows(rng, 1), (T + 70, 1))
    cases["all train rows equal"] = (rand_rows(rng, 66), t)
    return cases


@pytest.mark.parametrize("lanes", LANES)
def test_ties(lanes_ctx, K, lanes):
    cases = tie_cases(K.TILE)
    qs, ts = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    lanes_ctx.set_knn_lanes(lanes)
    got = K.knn2_hamming_batch(lanes_ctx, qs, ts)
    assert_pairs_equal(got, qs, ts, f"lanes {lanes}")
    # what the cases are there for, on the device's answer
    T = K.TILE
    gi, gd = got[0]
    assert gi[0].tolist() == [5, T + 17] and gd[0].tolist() == [0, 0] and gi[1].tolist() == [5, T + 17] and gd[1].tolist() == [2, 2]
    gi, gd = got[1]
    assert gi[:4].tolist() == [[10, 11], [20, 25], [40, 77], [3, 130]] and not gd[:4].any() and gd[4].tolist() == [1, 1]
    gi, gd = got[2]
    assert gi.tolist() == [[T - 1, T + 2], [2, T + 1], [T - 1, T + 2]] and gd[2].tolist() == [1, 1]
    assert got[3][1][:, 0].tolist() == [0, 0, 0] and got[3][0][:, 0].tolist() == [69, 0, 33]
    assert (got[4][0] == [0, 1]).all() and (got[4][1][:, 0] == got[4][1][:, 1]).all()


def mixed_batch():
    rng = np.random.default_rng(3)
    sizes = [(70, 300), (0, 50), (33, 0), (5, 1), (257, 1030), (1, 2), (64, 64), (300, 300)]
    return [rand_rows(rng, a) for a, _ in sizes], [rand_rows(rng, b) for _, b in sizes]


@pytest.mark.parametrize("lanes", LANES)
def test_batch_equals_single_calls(lanes_ctx, K, lanes):
    qs, ts = mixed_batch()
    lanes_ctx.set_knn_lanes(lanes)
    got = K.knn2_hamming_batch(lanes_ctx, qs, ts)
    assert_pairs_equal(got, qs, ts, f"lanes {lanes}")
    for b in range(len(qs)):
        (si, sd), = K.knn2_hamming_batch(lanes_ctx, [qs[b]], [ts[b]])
        assert np.array_equal(si, got[b][0]) and np.array_equal(sd, got[b][1]), f"pair {b} alone differs from the batch"
    assert len(got[1][0]) == 0 and (got[2][0] == -1).all() and (got[2][1] == -1).all()      # no queries; no train rows
    assert (got[3][0] == [0, -1]).all() and (got[3][1][:, 1] == -1).all() and (got[3][1][:, 0] >= 0).all()   # one train row


@pytest.mark.parametrize("lanes", LANES)
def test_dev_form_equals_host_form(lanes_ctx, K, lanes):
    qs, ts = mixed_batch()
    lanes_ctx.set_knn_lanes(lanes)
    host = K.knn2_hamming_batch(lanes_ctx, qs, ts)
    di, dd = K.knn2_hamming_batch_dev(lanes_ctx, qs, ts)
    assert np.array_equal(di, np.concatenate([h[0] for h in host])) and np.array_equal(dd, np.concatenate([h[1] for h in host]))


def test_two_pairs_of_2048(lanes_ctx, K):
    rng = np.random.default_rng(4)
    qs, ts = [rand_rows(rng, 2048) for _ in range(2)], [rand_rows(rng, 2048) for _ in range(2)]
    ts[1][2047] = ts[1][0]          # a tie between the first and the last row of a pair
    qs[1][7] = ts[1][0]
    got = K.knn2_hamming_batch(lanes_ctx, qs, ts)
    assert_pairs_equal(got, qs, ts)
    assert got[1][0][7].tolist() == [0, 2047]


def test_untouched_slots_and_row_limit_of_the_dev_form(lanes_ctx, K):
    """total_query below d_q_off[B]: the rows beyond it keep what the caller put there; a missing neighbour is -1 / -1"""
    rng = np.random.default_rng(5)
    qs, ts = [rand_rows(rng, 40), rand_rows(rng, 30), rand_rows(rng, 20)], [rand_rows(rng, 90), rand_rows(rng, 1), rand_rows(rng, 70)]
    ctx = lanes_ctx
    q, t = np.concatenate(qs), np.concatenate(ts)
    qo, to = np.array([0, 40, 70, 90], np.int32), np.array([0, 90, 91, 161], np.int32)
    ref = R.knn2_batch(qs, ts)
    for lanes in LANES:
        ctx.set_knn_lanes(lanes)
        d = [ctx.to_device(a) for a in (qo, to, q, t, np.full((90, 2), -7, np.int32), np.full((90, 2), -7, np.int32))]
        st = ctx.lib.ov2_knn2_hamming_batch_dev(ctx.h, 3, 75, *[a.ptr for a in d])
        assert st == 0
        ctx.synchronize()
        gi, gd = d[4].get(), d[5].get()
        assert (gi[75:] == -7).all() and (gd[75:] == -7).all(), f"lanes {lanes}: rows beyond total_query were written"
        assert np.array_equal(gi[:40], ref[0][0]) and np.array_equal(gd[:40], ref[0][1])
        assert np.array_equal(gi[40:70], ref[1][0]) and (gi[40:70, 1] == -1).all() and (gd[40:70, 1] == -1).all()
        assert np.array_equal(gi[70:75], ref[2][0][:5]) and np.array_equal(gd[70:75], ref[2][1][:5])


def test_refusals(lanes_ctx, K):
    ctx, L = lanes_ctx, lanes_ctx.lib
    vp = C.c_void_p
    INVALID = -1
    q, t = np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8)
    idx, dist = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.int32)
    P = lambda a: a.ctypes.data_as(vp)
    one = lambda v: np.array([v], np.int32)

    def host(B, nq, nt, q_=q, t_=t, i_=idx, d_=dist):
        return L.ov2_knn2_hamming_batch(ctx.h, B, None if nq is None else P(nq), None if nt is None else P(nt),
                                        None if q_ is None else P(q_), None if t_ is None else P(t_),
                                        None if i_ is None else P(i_), None if d_ is None else P(d_))

    assert host(0, None, None, None, None, None, None) == 0                       # B = 0
    assert host(1, one(0), one(4)) == 0 and host(1, one(0), one(0), None, None, None, None) == 0   # nothing to do
    assert host(-1, one(4), one(4)) == INVALID
    assert host(1, None, one(4)) == INVALID and host(1, one(4), None) == INVALID
    assert host(1, one(-1), one(4)) == INVALID and host(1, one(4), one(-1)) == INVALID
    assert host(1, one(4), one(4), None) == INVALID and host(1, one(4), one(4), q, None) == INVALID
    assert host(1, one(4), one(4), q, t, None) == INVALID and host(1, one(4), one(4), q, t, idx, None) == INVALID
    assert host(1, one(4), one(K.MAX_TRAIN + 1)) == INVALID                       # checked before any row is read
    assert host(1, one(K.MAX_ROWS + 1), one(4)) == INVALID
    big = np.zeros(K.MAX_BATCH + 1, np.int32)
    assert host(K.MAX_BATCH + 1, big, big) == INVALID
    two = np.array([K.MAX_TRAIN, K.MAX_TRAIN], np.int32)
    many = np.full(K.MAX_ROWS // K.MAX_TRAIN + 1, K.MAX_TRAIN, np.int32)          # every pair within its limit, the sum above
    assert host(len(many), np.zeros(len(many), np.int32), many) == INVALID and len(two) == 2
    assert L.ov2_knn2_hamming_batch(None, 0, None, None, None, None, None, None) == INVALID
    # device form
    d = [ctx.to_device(a) for a in (np.array([0, 4], np.int32), np.array([0, 4], np.int32), q, t, idx, dist)]
    p = [a.ptr for a in d]
    dev = lambda B, n, *a: L.ov2_knn2_hamming_batch_dev(ctx.h, B, n, *a)
    assert dev(0, 0, None, None, None, None, None, None) == 0 and dev(1, 0, *p) == 0
    assert dev(-1, 4, *p) == INVALID and dev(1, -4, *p) == INVALID
    assert dev(K.MAX_BATCH + 1, 4, *p) == INVALID and dev(1, K.MAX_ROWS + 1, *p) == INVALID
    for k in (0, 1, 2, 4, 5):
        a = list(p)
        a[k] = None
        assert dev(1, 4, *a) == INVALID, f"null argument {k}"
    assert dev(0, 4, *p) == INVALID                                               # rows without a pair
    a = list(p)
    a[2] = vp(p[2].value + 8)
    assert dev(1, 4, *a) == INVALID                                               # misaligned descriptors
    a = list(p)
    a[3] = vp(p[3].value + 4)
    assert dev(1, 4, *a) == INVALID
    for bad in (-1, 2, 3, 8, 32, 128):
        assert L.ov2_knn_set_lanes(ctx.h, bad) == INVALID
    assert L.ov2_knn_set_lanes(None, 0) == INVALID
    ctx.synchronize()
    assert dev(1, 4, *p) == 0                                                     # the context still works
    ctx.synchronize()
    assert (d[4].get() == [0, 1]).all()
