"""The loop detector without a GPU: the checker tests/lcd_ref.py against examples worked by hand from binary_index.cc,
lcdetector.cc and island.h, its behaviour on the seeded streams of ov2slam_amd/synth_lcd.py, and the C++ host detector with the
brute-force back end (no context) against the checker on every stream."""
import math

import numpy as np
import pytest

import lcd_ref as R

SMALL = dict(p=5, island_size=4, nframes_after_lc=3)
SEED = 1
MARGIN = 1e-9


def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(row, *bits):
    r = row.copy()
    for bit in bits:
        r[bit // 8] ^= np.uint8(1 << (bit % 8))
    return r


def make_streams():
    from ov2slam_amd import synth_lcd as S
    return {"revisit": (S.stream(SEED), S.planted()),
            "no revisit": (S.stream(SEED + 100, revisit_from=None), {}),
            "empty keyframes": (S.stream(SEED + 200, empty=(12, 33)), S.planted())}


@pytest.fixture(scope="module")
def streams():
    return make_streams()


@pytest.fixture(scope="module")
def checked(streams):
    """the checker's run of every stream, computed once: name -> (run_stream output, image-to-keyframe list, trace)"""
    out = {}
    for name, (st, _) in streams.items():
        det = R.LCDetector(R.Params(**SMALL))
        run, kf_of = R.run_stream(det, st)
        out[name] = (run, kf_of, det.trace)
    return out


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from ov2slam_amd import lcd
    return lcd


# ---- worked by hand ---------------------------------------------------------------------------------------------------------

def test_tfidf_three_images_by_hand():
    rng = np.random.default_rng(11)
    A, B, Cc, D = rand_rows(rng, 4)
    ix = R.ImageIndex(purge_descriptors=False)
    ix.add_image(0, [A, B])                                                    # words 0 (A), 1 (B)
    ix.add_image(1, [flipped(A, 1), Cc], [(0, 0, 1)])                          # word 2 (C); word 0 seen in image 1
    ix.add_image(2, [flipped(B, 2), flipped(Cc, 3), D, flipped(B, 4)], [(0, 1, 1), (1, 2, 1), (3, 1, 1)])   # word 3 (D)
    assert sorted(ix.words) == [0, 1, 2, 3] and ix.nimages == 3
    assert [(i[0], i[1]) for i in ix.words[1][1]] == [(0, 1), (2, 0), (2, 3)]   # (image, keypoint) items of word 1
    # a query of 4 rows whose kept matches are word 0, word 1, word 0
    score = ix.search_images(4, [(0, 0, 5), (1, 1, 7), (2, 0, 9)])
    L = math.log(3.0 / 2.0)      # words 0 and 1 are each seen in 2 of the 3 images
    w0, w1 = (2.0 / 4) * L, (1.0 / 4) * L
    # match 1 (word 0: items in images 0, 1), match 2 (word 1: items in images 0, 2, 2 -- once per ITEM), match 3 (word 0 again)
    assert score == [(w0 + w1) + w0, w0 + w0, w1 + w1]
    assert score[0] == pytest.approx(1.25 * L, rel=1e-15) and score[2] == pytest.approx(0.5 * L, rel=1e-15)


def test_islands_by_hand():
    isl = R.build_islands([(10, 1.0), (11, 0.5)], 4)                            # 11 fits [8, 12]
    assert [s.tuple() for s in isl] == [(10, 8, 12, 1.5 / 5)]
    # 14 is right of [8, 12]: its lower limit 12 is clipped to 13; 6 is left of it: its upper limit 8 is clipped to 7
    isl = R.build_islands([(10, 1.0), (14, 0.9), (6, 0.6)], 4)
    assert [s.tuple() for s in isl] == [(14, 13, 16, 0.9 / 4), (10, 8, 12, 1.0 / 5), (6, 4, 7, 0.6 / 4)]
    assert [s.tuple() for s in R.build_islands([(1, 1.0)], 4)] == [(1, 0, 3, 1.0 / 4)]   # id below island_offset: clamped at 0
    # equal island scores: the lower img_id first (1.0 / 5 and 0.8 / 4 are the same double)
    assert 1.0 / 5 == 0.8 / 4
    assert [s.img_id for s in R.build_islands([(14, 0.8), (10, 1.0)], 4)] == [10, 14]


def test_overlap_with_the_last_island_beats_a_better_score():
    rng = np.random.default_rng(12)
    det = R.LCDetector(R.Params(p=2, island_size=4, nframes_after_lc=0, purge_descriptors=False))   # p = 2: the query itself stays out
    base = [rand_rows(rng, 6) for _ in range(30)]
    for i, d in enumerate(base):
        det.process(i, d)
    det.last_island = R.Island(9, 0.4, 8, 12)
    # the query shares 4 rows with image 22 and 2 with image 10: image 22's island scores higher, image 10's overlaps the last
    q = np.stack([flipped(base[22][k], 5) for k in range(4)] + [flipped(base[10][k], 6) for k in range(2)])
    st, train = det.process(30, q)
    isl = det.trace[-1]["islands"]
    assert st == R.LC_DETECTED and [s[0] for s in isl][:2] == [22, 10] and isl[0][3] > isl[1][3]
    assert train == 10 and (det.last_island.min_img_id, det.last_island.max_img_id) == (8, 12)


def purge_images():
    rng = np.random.default_rng(13)
    A, B, Cc, D, E = rand_rows(rng, 5)
    return [np.stack([A, B]), np.stack([flipped(A, 1, 2, 3), Cc]), D[None], E[None]]


def test_purge_by_hand(host):
    """word B (seen once, image 0) is gone after two more images, word A (seen twice) stays, word C goes one image later, and
    the ids go on counting"""
    imgs = purge_images()
    det = R.LCDetector(R.Params(p=1, nframes_after_lc=100))
    hd = host.Detector(None, p=1, nframes_after_lc=100)
    want = [([0, 1], [], []), ([2], [], [(0, 0, 3)]), ([3], [1], []), ([4], [2], [])]
    for i, (d, (added, purged, add_matches)) in enumerate(zip(imgs, want)):
        det.process(i, d)
        t = det.trace[-1]
        assert (t["added"], t["purged"], t["add_matches"]) == (added, purged, add_matches)
        hd.process(i, d)
        ht = hd.trace()
        assert (ht["added"], ht["purged"], ht["add_matches"]) == (added, purged, add_matches)
    assert sorted(det.index.words) == [0, 3, 4] and hd.counts()["words"] == 3 and hd.counts()["images"] == 4
    assert [(i[0], i[1]) for i in det.index.words[0][1]] == [(0, 0), (1, 0)]


def test_nan_path(host):
    """max == min in filterCandidates: 0 / 0 is NaN, no candidate passes, no islands"""
    rng = np.random.default_rng(14)
    a = rand_rows(rng, 8)
    for mk in (lambda: R.LCDetector(R.Params(p=2, nframes_after_lc=0)), lambda: host.Detector(None, p=2, nframes_after_lc=0)):
        det = mk()
        assert det.process(0, a) == (R.LC_NOT_ENOUGH_IMAGES, 0)
        # one image indexed, and every query row matches it: its score is the only one
        assert det.process(1, np.stack([flipped(r, 9) for r in a])) == (R.LC_NOT_ENOUGH_ISLANDS, 0)
        tr = det.trace[-1] if isinstance(det, R.LCDetector) else det.trace()
        assert len(tr["matches"]) == 8 and len(tr["scores"]) == 1 and tr["islands"] == []
    det = R.LCDetector(R.Params(p=3, nframes_after_lc=0))
    hd = host.Detector(None, p=3, nframes_after_lc=0)
    for i in range(5):                  # images 0 .. 2 indexed when image 4 asks; nothing matches: all scores 0, NaN, no islands
        d = rand_rows(rng, 8)
        r = det.process(i, d)
        assert hd.process(i, d) == r
    assert r == (R.LC_NOT_ENOUGH_ISLANDS, 0) and det.trace[-1]["scores"] == [0.0, 0.0, 0.0] and det.trace[-1]["matches"] == []


# ---- seeded streams ----------------------------------------------------------------------------------------------------------

def test_streams_are_what_the_tests_need(streams):
    st, planted = streams["revisit"]
    assert len(st) == 40 and all(48 <= len(d) <= 64 for d in st) and planted[30] == 8 and planted[39] == 17
    st, _ = streams["empty keyframes"]
    assert [k for k, d in enumerate(st) if len(d) == 0] == [12, 33]


def test_checker_finds_the_planted_keyframes(streams, checked):
    for name in ("revisit", "empty keyframes"):
        st, planted = streams[name]
        run, kf_of, _ = checked[name]
        seen = 0
        for kf, img, status, train in run:
            if kf in planted and len(st[planted[kf]]) and status in (R.LC_DETECTED, R.LC_NOT_ENOUGH_ISLANDS):   # the gate was open
                assert status == R.LC_DETECTED, (name, kf)
                assert abs(kf_of[train] - planted[kf]) <= SMALL["island_size"] // 2, (name, kf, kf_of[train])
                seen += 1
        assert seen >= 2   # the gate opens on every third revisit keyframe; one planted keyframe of the last stream is empty
    run, kf_of, _ = checked["empty keyframes"]
    assert [kf for kf, *_ in run] == [k for k in range(40) if k not in (12, 33)] and [img for _, img, *_ in run] == list(range(38))


def test_checker_never_returns_a_neighbour_without_a_revisit(checked):
    run, kf_of, _ = checked["no revisit"]
    hits = [(kf, kf_of[train]) for kf, img, status, train in run if status == R.LC_DETECTED]
    assert hits and all(abs(a - b) > 3 for a, b in hits)


def test_every_decision_margin_is_wide(checked):
    for name, (_, _, trace) in checked.items():
        assert min(t["margin"] for t in trace) > MARGIN, name


def assert_trace_equal(ht, t, what):
    assert ht["add_matches"] == t["add_matches"] and ht["matches"] == t["matches"], what
    assert ht["added"] == t["added"] and ht["purged"] == t["purged"], what
    assert len(ht["scores"]) == len(t["scores"]) and len(ht["islands"]) == len(t["islands"]), what
    for a, b in zip(ht["scores"], t["scores"]):
        assert abs(a - b) <= 1e-12 * abs(b), what
    for a, b in zip(ht["islands"], t["islands"]):
        assert tuple(a[:3]) == tuple(b[:3]) and abs(a[3] - b[3]) <= 1e-12 * abs(b[3]), what


def test_host_detector_equals_the_checker(host, streams, checked):
    for name, (st, _) in streams.items():
        run, _, trace = checked[name]
        hd = host.Detector(None, **SMALL)
        for (kf, img, status, train), t in zip(run, trace):
            assert hd.process(img, st[kf]) == (status, train), (name, kf)
            assert_trace_equal(hd.trace(), t, (name, kf))
            assert hd.counts()["words"] == t["nwords"]
