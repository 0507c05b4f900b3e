"""ov2_match_pairs_dev: the output of the batched local-map matcher as the ordered pair lists of Mapper::mergeMatches
(reference src/mapper.cpp:556-574: map_previd_newid walked in ascending prevlmid), on the device -- against the sorted numpy
gather, exactly: counts, pairs and the -1 fill -- and the chain pairs -> ov2_map_merge_points_batch_dev against the
host-pointer merge fed the numpy pairs."""
import ctypes as C

import numpy as np
import pytest

from ov2slam_amd import device_map as DM, mapper, synth_match
from test_merge_ref_cpu import MAPS, the_map, full_list
from test_map_merge_gpu import fresh, same_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def numpy_pairs(kp_off, cand_off, kp_lmid, cand_lmid, mc):
    """per frame the (prev, new) pairs in ascending prev; returns (prev, new: n_kp each, -1 behind the pairs; counts)"""
    prev, new = np.full(len(kp_lmid), -1, np.int32), np.full(len(kp_lmid), -1, np.int32)
    cnt = np.zeros(len(kp_off) - 1, np.int32)
    for b in range(len(cnt)):
        k0, k1 = kp_off[b], kp_off[b + 1]
        ks = k0 + np.flatnonzero(mc[k0:k1] >= 0)
        ks = ks[np.argsort(kp_lmid[ks], kind="stable")]
        cnt[b] = len(ks)
        prev[k0:k0 + len(ks)] = kp_lmid[ks]
        new[k0:k0 + len(ks)] = cand_lmid[cand_off[b] + mc[ks]]
    return prev, new, cnt


def device_pairs(ctx, kp_off, cand_off, kp_lmid, cand_lmid, mc):
    """ov2_match_pairs_dev on uploaded arrays: (DevPairs, the uploads to keep alive)"""
    i32 = lambda a: ctx.to_device(np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32))
    up = [i32(kp_off), i32(cand_off), i32(kp_lmid), i32(cand_lmid), i32(mc)]
    n, B = len(kp_lmid), len(kp_off) - 1
    d_prev, d_new = ctx.to_device(np.full(max(n, 1), -7, np.int32)), ctx.to_device(np.full(max(n, 1), -7, np.int32))
    d_np = ctx.to_device(np.full(B, -7, np.int32))
    assert ctx.lib.ov2_match_pairs_dev(ctx.h, B, n, *[u.ptr for u in up], d_prev.ptr, d_new.ptr, d_np.ptr) == 0
    return DM.DevPairs(kp_off, d_prev, d_new, d_np), up


def test_pairs_equal_the_sorted_gather(ctx):
    """three frames: no match at all; matches whose kp_lmid descend (and one keypoint without a match between them); a single
    keypoint.  A fourth, of 700 keypoints, takes the kernel's loops over more than one 256-wide chunk"""
    rng = np.random.default_rng(3)
    big = rng.permutation(5000)[:700].astype(np.int32)
    kp_lmid = np.concatenate([[11, 12, 13, 14, 15], [90, 80, 70, 60, 50, 40], [7], big]).astype(np.int32)
    kp_off = np.array([0, 5, 11, 12, 712], np.int32)
    cand_lmid = np.concatenate([[100, 101, 102], [200, 201, 202, 203, 204, 205, 206], [300, 301], 1000 + np.arange(900)]).astype(np.int32)
    cand_off = np.array([0, 3, 10, 12, 912], np.int32)
    mc = np.concatenate([[-1] * 5, [3, 0, -1, 6, 1, 2], [1], np.where(rng.random(700) < 0.6, rng.integers(0, 900, 700), -1)]).astype(np.int32)
    dp, keep = device_pairs(ctx, kp_off, cand_off, kp_lmid, cand_lmid, mc)
    ctx.synchronize()
    prev, new, cnt = numpy_pairs(kp_off, cand_off, kp_lmid, cand_lmid, mc)
    assert cnt.tolist()[:3] == [0, 5, 1] and cnt[3] > 256
    assert prev[5:11].tolist() == [40, 50, 60, 80, 90, -1] and new[5:11].tolist() == [202, 201, 206, 200, 203, -1]
    assert np.array_equal(dp.d_n_pairs.get(), cnt)
    assert np.array_equal(dp.d_prev.get(), prev) and np.array_equal(dp.d_new.get(), new)
    # B = 0 enqueues nothing; negative counts are refused
    assert ctx.lib.ov2_match_pairs_dev(ctx.h, 0, 0, *([None] * 8)) == 0
    assert ctx.lib.ov2_match_pairs_dev(ctx.h, -1, 0, *([None] * 8)) == -1


def test_pairs_step_of_a_matcher_run(ctx):
    """MatchBatchInputDev.pairs() behind a real ov2_match_to_map_batch_dev run, with seeded lmids"""
    F = synth_match.make_frames()
    inp = synth_match.batch_input([F["plain_a"], F["no_kp"], F["plain_b"]])
    rng = np.random.default_rng(1)
    kp_lmid = rng.permutation(100000)[:inp.c.n_kp].astype(np.int32)
    cand_lmid = (100000 + rng.permutation(100000)[:inp.c.n_cand]).astype(np.int32)
    d = mapper.MatchBatchInputDev(ctx, inp)
    d.enqueue()
    dp = d.pairs(kp_lmid, cand_lmid)
    mc, _ = d.get()
    prev, new, cnt = numpy_pairs(inp.kp_off, inp.cand_off, kp_lmid, cand_lmid, mc)
    assert cnt[0] > 0 and cnt[1] == 0 and cnt[2] > 0
    n = inp.c.n_kp
    assert np.array_equal(dp.d_n_pairs.get(), cnt) and np.array_equal(dp.d_prev.get()[:n], prev) and np.array_equal(dp.d_new.get()[:n], new)


def test_pairs_then_merge_equals_the_host_pointer_merge(ctx):
    """match_cand -> ov2_match_pairs_dev -> ov2_map_merge_points_batch_dev on the small and the large map (hand-written
    match_cand arrays, no matcher run) == ov2_map_merge_points_batch fed the numpy pairs"""
    kp_lmid, cand_lmid, mc, kp_off, cand_off = [], [], [], [0], [0]
    for key in MAPS:
        pairs = full_list(*key)[0]
        nl = key[1]
        pairs = pairs[(pairs.min(1) >= 0) & (pairs.max(1) < nl)]
        _, first = np.unique(pairs[:, 0], return_index=True)     # a frame holds a landmark once
        pairs = pairs[np.sort(first)]
        rng = np.random.default_rng(key[1])
        extra = np.setdiff1d(np.arange(nl), pairs[:, 0])[:7]      # keypoints without a match
        lm = np.concatenate([pairs[:, 0], extra])
        m = np.concatenate([np.arange(len(pairs)), np.full(len(extra), -1)])
        o = rng.permutation(len(lm))
        kp_lmid.append(lm[o]); mc.append(m[o]); cand_lmid.append(pairs[:, 1])
        kp_off.append(kp_off[-1] + len(lm)); cand_off.append(cand_off[-1] + len(pairs))
    kp_lmid, cand_lmid, mc = (np.concatenate(a).astype(np.int32) for a in (kp_lmid, cand_lmid, mc))
    kp_off, cand_off = np.array(kp_off, np.int32), np.array(cand_off, np.int32)
    prev, new, cnt = numpy_pairs(kp_off, cand_off, kp_lmid, cand_lmid, mc)
    assert cnt[0] > 20 and cnt[1] > 256
    maps, twins = [fresh(ctx, k) for k in MAPS], [fresh(ctx, k) for k in MAPS]
    try:
        dp, keep = device_pairs(ctx, kp_off, cand_off, kp_lmid, cand_lmid, mc)
        hdr, st = DM.merge_points_batch(ctx, maps, dp, dev=True)
        lists = [np.stack([prev[kp_off[b]:kp_off[b] + cnt[b]], new[kp_off[b]:kp_off[b] + cnt[b]]], 1) for b in range(2)]
        hdr2, st2 = DM.merge_points_batch(ctx, twins, lists)
        for b in range(2):
            assert hdr[b] == hdr2[b] and hdr[b]["n_pairs"] == cnt[b] and hdr[b]["n_rows_moved"] > 0
            assert np.array_equal(st[b][:cnt[b]], st2[b]) and np.all(st[b][cnt[b]:] == DM.MERGE_NOT_RUN)
            assert same_tables(maps[b].download(), twins[b].download())
    finally:
        for m in maps + twins:
            m.close()
