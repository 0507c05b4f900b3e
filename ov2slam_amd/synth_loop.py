"""A seeded revisit scene for the loop-candidate matcher (ov2::LoopCloser, the 2D-2D half of processLoopCandidate): one map
whose new keyframes see places that much older keyframes saw, under DIFFERENT lmids, so that only the descriptors of the map
points and the two-view geometry of the keypoints tell that it is the same place.  Data only: who observes what, pixels,
descriptors.  Seeded, deterministic.

Keyframes and the candidate pairs (new keyframe, candidate) of `pairs`, by name:
  clean     (40, 2)    the revisit: true matches, every smaller effect listed in `effects`, wrong-but-accepted matches
  covisible (40, 39)   covisibility score 31: skipped before any matching
  cov30     (40, 38)   score 30: not skipped; too few matches
  few       (40, 5)    8 true matches: stops at the < 15 gate
  nogeom    (40, 7)    20 accepted matches whose pixels in the candidate are random: the 5-point filter fails
  walkdown  (40, 9)    keyframes 9 and 8 are not in the map: the candidate becomes 7
  empty     (40, 6)    the candidate has no 3D keypoint: the early return, no query reaches the matcher
  edge_odd  (50, 3), edge_even (51, 4), edge_max (52, 10)   the ratio test and maxdist at their edges, see _edge_pair
The descriptors of ordinary map points are random 256-bit strings: two of them are 128 +- 8 bits apart, so a true match
(at most 10 flipped bits) passes the ratio test and an unrelated query does not."""
import numpy as np

from . import synth_ba
from .synth_epi import K_EUROC

W, H = 752, 480
RATIO_EDGES = [(17, 20), (34, 40), (51, 60), (68, 80), (85, 100), (102, 120)]
NEW, CLEAN, COV, COV30, FEW, NOGEOM, WALK, EMPTY = 40, 2, 39, 38, 5, 7, 9, 6


def ratio_edge_targets():
    """every edge pair (d0, d1) and its four neighbours at distance 1"""
    out = []
    for d0, d1 in RATIO_EDGES:
        out += [(d0, d1), (d0 - 1, d1), (d0 + 1, d1), (d0, d1 - 1), (d0, d1 + 1)]
    return out


def flip(desc, bits):
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _project(K, X):
    return (K[:2] * X[:, :2] / X[:, 2:3] + K[2:]).astype(np.float32)


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kps = {}        # kfid -> list of (lmid, (u, v), kp3d)
        self.desc = {}       # lmid -> (32,) uint8; absent = a map point without a descriptor
        self.forget_lm = []  # lmids whose map point is dropped once the keypoints are in place
        self.next_lmid = 100

    def lmid(self):
        self.next_lmid += 1
        return self.next_lmid

    def rand_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def rand_px(self):
        return self.rng.uniform([20, 20], [W - 20, H - 20]).astype(np.float32)

    def kp(self, kfid, lmid, px, kp3d, desc=None):
        self.kps.setdefault(kfid, []).append((int(lmid), (float(px[0]), float(px[1])), bool(kp3d)))
        if desc is not None:
            self.desc[int(lmid)] = np.array(desc, np.uint8)
        return int(lmid)


def _edge_pair(b, newkf, lckf, H_bits, targets):
    """A pair whose train set is two rows, a and b = a with the H_bits bits of h flipped.  A query that has to see them at
    (d0, d1) is a with d0 bits flipped, o = (d0 + H_bits - d1) / 2 of them inside h: its distance to b is d0 + H_bits - 2 o."""
    a = b.rand_desc()
    h = list(range(256 - H_bits, 256))
    ida = b.kp(lckf, b.lmid(), b.rand_px(), True, a)
    idb = b.kp(lckf, b.lmid(), b.rand_px(), True, flip(a, h))
    out = []
    for d0, d1 in targets:
        assert (d0 + H_bits - d1) % 2 == 0 and d1 >= d0
        o = (d0 + H_bits - d1) // 2
        assert 0 <= o <= min(d0, H_bits) and d0 - o <= 256 - H_bits
        g = h[:o] + list(range(d0 - o))
        q = b.kp(newkf, b.lmid(), b.rand_px(), True, flip(a, g))
        out.append(dict(query=q, d0=d0, d1=d1, first=ida if d0 <= d1 else idb))
    return out


def make_scene(seed=0, n_true=60):
    b = _Builder(seed)
    rng = b.rng
    K = np.asarray(K_EUROC, np.float64)
    # the revisit: the candidate keyframe at the origin, the new keyframe at (R, t); X in front of both
    axis = rng.normal(size=3)
    R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), np.deg2rad(6.0) * axis / np.linalg.norm(axis)]))
    t = np.array([0.35, -0.1, 0.08])
    n_pts = n_true + 64
    X = np.stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(2.5, 12, n_pts)], 1)
    px_lc = _project(K, X) + rng.normal(0, 0.25, (n_pts, 2)).astype(np.float32)
    px_new = _project(K, (X - t) @ R) + rng.normal(0, 0.25, (n_pts, 2)).astype(np.float32)
    eff = {k: [] for k in ("true", "distractor_query", "distractor_train", "ambiguous", "tie_far", "tie_exact", "shared3d", "shared2d",
                           "no_desc", "absent", "wrong")}
    true_pairs, wrong_pairs = set(), set()
    pt = iter(range(n_pts))
    lc_rows = []   # keypoints of the candidate, shuffled before they are added so that train rows of one effect lie far apart

    # true matches: the same 3D point under two lmids, the candidate's descriptor = the new one's with 0..10 flipped bits
    true_q = []
    for _ in range(n_true):
        i = next(pt)
        d = b.rand_desc()
        q = b.kp(NEW, b.lmid(), px_new[i], rng.random() < 0.7, d)
        l = b.lmid()
        lc_rows.append((l, px_lc[i], flip(d, rng.choice(256, int(rng.integers(0, 11)), replace=False))))
        eff["true"].append(q)
        true_pairs.add((q, l))
        true_q.append((q, d, i))
    # wrong but accepted: the candidate's keypoint with the matching descriptor looks at another point
    for _ in range(8):
        i, j = next(pt), next(pt)
        d = b.rand_desc()
        q = b.kp(NEW, b.lmid(), px_new[i], True, d)
        l = b.lmid()
        lc_rows.append((l, px_lc[j] + np.float32([60, -45]), flip(d, rng.choice(256, 4, replace=False))))
        eff["wrong"].append(q)
        wrong_pairs.add((q, l))
    # distractors on both sides
    for _ in range(12):
        eff["distractor_query"].append(b.kp(NEW, b.lmid(), b.rand_px(), rng.random() < 0.5, b.rand_desc()))
    for _ in range(40):
        l = b.lmid()
        lc_rows.append((l, b.rand_px(), b.rand_desc()))
        eff["distractor_train"].append(l)
    # ambiguous: two train rows 6 and 7 bits from the query (6 <= 7 * 0.85 is false)
    for _ in range(6):
        d = b.rand_desc()
        eff["ambiguous"].append(b.kp(NEW, b.lmid(), b.rand_px(), True, d))
        bits = rng.choice(256, 13, replace=False)
        lc_rows.append((b.lmid(), b.rand_px(), flip(d, bits[:6])))
        lc_rows.append((b.lmid(), b.rand_px(), flip(d, bits[6:])))
    # exact ties at 5 bits (rejected; neighbour 0 is the lower row) and exact copies (0 <= 0 * 0.85: accepted, the lower row)
    tie_rows = []
    for k in range(6):
        d = b.rand_desc()
        q = b.kp(NEW, b.lmid(), b.rand_px(), True, d)
        bits = rng.choice(256, 10, replace=False)
        rows = (flip(d, bits[:5]), flip(d, bits[5:])) if k < 3 else (d.copy(), d.copy())
        l0, l1 = b.lmid(), 9000 + 37 * k
        tie_rows.append(((l0, b.rand_px(), rows[0]), (l1, b.rand_px(), rows[1])))
        eff["tie_far" if k < 3 else "tie_exact"].append(q)
    # keypoints of both keyframes under ONE lmid: 3D in the new keyframe -> identity pairs; 2D there -> a query like any other
    for k in range(14):
        i = next(pt)
        l = b.lmid()
        is3d = k < 8
        b.kp(NEW, l, px_new[i], is3d, b.rand_desc())
        lc_rows.append((l, px_lc[i], None))
        eff["shared3d" if is3d else "shared2d"].append(l)
    # map points without a descriptor, and keypoints whose map point is gone, on both sides
    for _ in range(5):
        eff["no_desc"].append(b.kp(NEW, b.lmid(), b.rand_px(), True))
        l = b.lmid()
        lc_rows.append((l, b.rand_px(), None))
        eff["no_desc"].append(l)
    for _ in range(5):
        l = b.kp(NEW, b.lmid(), b.rand_px(), True, b.rand_desc())
        l2 = b.lmid()
        lc_rows.append((l2, b.rand_px(), b.rand_desc()))
        eff["absent"] += [l, l2]
        b.forget_lm += [l, l2]
    order = rng.permutation(len(lc_rows))
    for k in order:
        l, px, d = lc_rows[k]
        b.kp(CLEAN, l, px, True, d if l not in b.desc else None)
    for first, second in tie_rows:   # the two rows of a tie go in far apart; where the mirror's iteration puts them is read back
        b.kp(CLEAN, *first[:2], True, first[2])
    for _ in range(30):
        b.kp(CLEAN, b.lmid(), b.rand_px(), False, b.rand_desc())    # 2D keypoints of the candidate: never train rows
    for first, second in tie_rows:
        b.kp(CLEAN, *second[:2], True, second[2])

    # the other candidates of keyframe NEW
    for kfid, n in ((FEW, 8), (NOGEOM, 20)):
        for q, d, i in true_q[:n]:
            px = px_lc[i] if kfid == FEW else b.rand_px()
            b.kp(kfid, b.lmid(), px, True, flip(d, rng.choice(256, 3, replace=False)))
        for _ in range(10):
            b.kp(kfid, b.lmid(), b.rand_px(), True, b.rand_desc())
    for kfid in (COV, COV30):
        for q, d, i in true_q[:5]:
            b.kp(kfid, b.lmid(), px_lc[i], True, flip(d, [1, 2]))
    for _ in range(6):
        b.kp(EMPTY, b.lmid(), b.rand_px(), False, b.rand_desc())
    # the ratio test and maxdist at their edges
    tg = ratio_edge_targets()
    edges = _edge_pair(b, 50, 3, 19, [x for x in tg if (x[1] - x[0]) % 2 == 1])
    edges += _edge_pair(b, 51, 4, 20, [x for x in tg if (x[1] - x[0]) % 2 == 0])
    maxd = _edge_pair(b, 52, 10, 127, [(127, 254), (128, 255), (129, 256)])

    kfids = sorted(b.kps)
    poses = {k: np.array([0.05 * k, 0, 0, 0, 0, 0, 1.0]) for k in kfids}
    kps = {k: dict(lmid=np.array([r[0] for r in v], np.int32), uv=np.array([r[1] for r in v], np.float32).reshape(-1, 2),
                   kp3d=np.array([r[2] for r in v], np.uint8)) for k, v in b.kps.items()}
    pairs = dict(clean=(NEW, CLEAN), covisible=(NEW, COV), cov30=(NEW, COV30), few=(NEW, FEW), nogeom=(NEW, NOGEOM),
                 walkdown=(NEW, WALK), empty=(NEW, EMPTY), edge_odd=(50, 3), edge_even=(51, 4), edge_max=(52, 10))
    return dict(K4=K, w=W, h=H, kfids=kfids, poses=poses, kps=kps, desc=b.desc, forget_lm=sorted(b.forget_lm),
                cov=[(NEW, COV, 31), (NEW, COV30, 30)], pairs=pairs, effects=eff, true_pairs=true_pairs, wrong_pairs=wrong_pairs,
                ratio_edges=edges, maxdist_edges=maxd, R=R, t=t)
