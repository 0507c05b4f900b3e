"""Seeded inputs of the loop closer's map matcher (LoopCloser::matchToMap, src/loop_closer.cpp:586-763): a new keyframe that
revisits a place mapped by an old pass.  Its keypoints carry NEW map points (keyframes 40..44), the local map of the loop
candidate holds the OLD ones (keyframes 0..24) at the true position plus millimetre noise, one descriptor per observing
keyframe, a few bits apart.  The projection pose is the true pose plus what a P3P on noisy pixels leaves (a few tenths of a
pixel), not the drifted pose the keyframe stores.

Pairs are dicts as loop_match.LoopMatchInput takes them: Twc, kps [px, matched, descs, kfids, lmid], cands [wpt, descs, kfids,
lmid].  The shapes are the smallest that still reach every path of the kernel (about 120 keypoints and 150 local-map points in
the general pairs): they are not EuRoC sizes.  Every planted effect is listed at its pair below and counted from the
checker's trace by tests/test_loop_verify_ref_cpu.py.

make_local_map_scene is the same revisit one level up: a whole map around the loop candidate (covisible keyframes inside and
outside its +- 15 window, one of them gone), from which LoopCloser::trackLoopLocalMap has to assemble those pair dicts itself;
track_jobs lists the calls the tests make on it.  Seeds are chosen on the checker alone."""
import numpy as np

from . import synth_ba

K4 = np.array([458.654, 457.296, 367.215, 248.375])
W, H, CELL = 752, 480, 35
FMAXPROJERR, FDISTRATIO = 10.0, 0.2 * 1.5        # trackLoopLocalMap(newkf, lckf, Twc, 10., fmax_desc_dist_ * 1.5, ...) (:269)
RADTAN = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)   # EuRoC cam0, for the lens-model case
OLD_KFS, NEW_KFS = 25, (40, 41, 42, 43, 44)


def _desc(rng, n=1):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(rng, d, nbits):
    d = d.copy()
    for f in rng.choice(256, size=nbits, replace=False):
        d[f >> 3] ^= np.uint8(1 << (f & 7))
    return d


class _Pair:
    """one (new keyframe, loop candidate) pair under construction"""

    def __init__(self, rng, lm0):
        self.rng = rng
        R, t = synth_ba.se3_exp(np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.15, 3)]))
        self.R, self.t = R, t
        self.Twc = synth_ba.pose7(R, t)
        self.kps, self.cands = [], []
        self.next_lm = lm0

    def _lm(self):
        self.next_lm += 1
        return self.next_lm

    def world(self, px, z):
        """the world point that projects (pinhole) to px at depth z"""
        cam = np.array([(px[0] - K4[2]) / K4[0] * z, (px[1] - K4[3]) / K4[1] * z, z])
        return self.R @ cam + self.t

    def kp(self, px, descs=None, kfids=None, matched=False):
        rng = self.rng
        if descs is None:
            descs = _desc(rng, int(rng.integers(1, 4)))
        if kfids is None:
            kfids = sorted(rng.choice(NEW_KFS, size=max(len(descs), 1), replace=False).tolist())
        self.kps.append(dict(px=np.float32(px), matched=bool(matched), descs=np.asarray(descs, np.uint8).reshape(-1, 32),
                             kfids=list(kfids), lmid=self._lm()))
        return len(self.kps) - 1

    def cand(self, wpt, descs, kfids=None):
        rng = self.rng
        if kfids is None:
            kfids = sorted(rng.choice(OLD_KFS, size=max(len(descs), 1), replace=False).tolist())
        self.cands.append(dict(wpt=np.asarray(wpt, np.float64), descs=np.asarray(descs, np.uint8).reshape(-1, 32), kfids=list(kfids),
                               lmid=self._lm()))
        return len(self.cands) - 1

    def revisit(self, k, nbits=(2, 12), px_off=(0.0, 0.0), ndesc=None):
        """the old map point of keypoint k's place: its descriptors are k's first descriptor a few bits apart, one per old
        observing keyframe, the closest of them NOT the first (MapPoint::desc_ is the first)"""
        rng, kp = self.rng, self.kps[k]
        n = int(rng.integers(2, 4)) if ndesc is None else ndesc
        base = kp["descs"][0] if len(kp["descs"]) else _desc(rng)[0]     # a keypoint whose map point is gone is still revisited
        ds = [_flip(rng, base, int(rng.integers(nbits[0] + 6, nbits[1] + 12)))] + \
             [_flip(rng, base, int(rng.integers(nbits[0], nbits[1]))) for _ in range(n - 1)]
        w = self.world(np.float64(kp["px"]) + np.asarray(px_off) + rng.normal(0, 0.3, 2), rng.uniform(3, 12)) + rng.normal(0, 0.002, 3)
        return self.cand(w, np.stack(ds))

    def dict(self):
        return dict(Twc=self.Twc, kps=self.kps, cands=self.cands)


def _general(rng, lm0, n_kp=120, n_cand=150, revisit_frac=0.55):
    """the plain revisit: about half of the local map re-observes a keypoint's place; the rest is unrelated, behind the
    camera, under z = 0.1, outside the image, without descriptor, co-observed; some keypoints are masked (already in the pair
    list), some have lost their map point"""
    P = _Pair(rng, lm0)
    for _ in range(n_kp):
        u = rng.uniform()
        px = (rng.uniform(2, W - 2), rng.uniform(2, H - 2))
        if u < 0.08:
            P.kp(px, matched=True)                            # vmatchedkpids
        elif u < 0.14:
            P.kp(px, descs=np.zeros((0, 32), np.uint8), kfids=[NEW_KFS[0]])   # map point gone / no descriptor
        else:
            P.kp(px)
    order = rng.permutation(n_kp)
    for c in range(n_cand):
        u = rng.uniform()
        k = int(order[c % n_kp])
        if u < revisit_frac:
            P.revisit(k)
        elif u < revisit_frac + 0.06:                         # same place, but co-observed in one keyframe: never a candidate
            kp = P.kps[k]
            P.cand(P.world(kp["px"], 5.0), kp["descs"][:1] if len(kp["descs"]) else _desc(rng), kfids=sorted({3, kp["kfids"][0]}))
        elif u < revisit_frac + 0.10:                         # behind the camera
            P.cand(P.R @ np.array([rng.normal(), rng.normal(), -rng.uniform(0.5, 3)]) + P.t, _desc(rng))
        elif u < revisit_frac + 0.13:                         # just under z = 0.1
            P.cand(P.R @ np.array([0.01 * rng.normal(), 0.01 * rng.normal(), 0.1 - rng.uniform(1e-4, 2e-3)]) + P.t, _desc(rng))
        elif u < revisit_frac + 0.17:                         # in front, outside the image
            P.cand(P.world((W + rng.uniform(1, 300), rng.uniform(0, H)) if rng.uniform() < 0.5 else (rng.uniform(0, W), -rng.uniform(1, 300)), 6.0),
                   _desc(rng))
        elif u < revisit_frac + 0.20:                         # no descriptor
            P.cand(P.world(P.kps[k]["px"], 5.0), np.zeros((0, 32), np.uint8), kfids=[1])
        else:                                                 # unrelated point somewhere in view
            P.cand(P.world((rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(3, 12)), _desc(rng, 2))
    return P


def _dense(rng, lm0):
    """a grid cell with 65 keypoints and one with 130 (the 64-lane chunk loop and the replay across chunks): the matches sit in
    the LAST keypoints of each cell, the ratio partner of one of them in the first chunk"""
    P = _Pair(rng, lm0)
    for (r, c, n, hits, tie) in ((5, 6, 65, (64, 3, 40), (1, 5)), (8, 12, 130, (128, 65, 3), (1, 129))):
        x0, y0 = c * CELL, r * CELL
        ks = [P.kp((x0 + rng.uniform(0.5, CELL - 0.5), y0 + rng.uniform(0.5, CELL - 0.5))) for _ in range(n)]
        for i in hits:
            P.revisit(ks[i])
        # two keypoints with the same descriptor (in the 130 cell: first and last chunk): the ratio rule rejects
        d = _desc(rng)[0]
        px = (x0 + 17.0, y0 + 17.0)
        P.kps[ks[tie[0]]].update(px=np.float32((px[0] + 2, px[1])), descs=d[None].copy())
        P.kps[ks[tie[1]]].update(px=np.float32((px[0] - 2, px[1])), descs=d[None].copy())
        P.cand(P.world(px, 6.0), _flip(rng, d, 5)[None])
    for _ in range(40):
        P.cand(P.world((rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(3, 12)), _desc(rng, 2))
    return P


def _borders(rng, lm0):
    """projections into the row 0 / column 0 cells and into the last cell; pxdist on either side of the 10 px gate; the
    view-angle gate; equal distances (ratio rule) and equal candidates (the later wins)"""
    P = _Pair(rng, lm0)
    for px in ((3.5, 4.5), (20.0, 200.5), (300.5, 12.0), (W - 1.5, H - 1.5), (W - 20.0, H - 30.0), (W - 3.0, 100.0), (200.0, H - 2.5)):
        k = P.kp(px)
        P.revisit(k)
    # either side of dmaxpxdist = 10 by 2e-2 px: the same descriptor, only the nearer one may match
    for dx, side in ((9.98, 1), (10.02, -1)):
        k = P.kp((400.0 + 60 * side, 240.0))
        P.cand(P.world((400.0 + 60 * side + dx, 240.0), 7.0), _flip(rng, P.kps[k]["descs"][0], 4)[None])
    # view angle: in front (z >= 0.1) but 4e4 m to the side: |z / norm| = 2.5e-6 under the reference's threshold of ~5.8e-6
    P.cand(P.R @ np.array([4.0e4, 0.0, 0.1001]) + P.t, _desc(rng))
    # two keypoints at the same distance from one candidate: 0.9 * second < best rejects
    d = _desc(rng)[0]
    P.kp((150.0, 300.0), descs=d[None].copy()), P.kp((153.0, 301.0), descs=d[None].copy())
    P.cand(P.world((151.0, 300.5), 5.0), _flip(rng, d, 6)[None])
    # two candidates at the same distance for one keypoint: the later one wins; an earlier, worse one loses
    k = P.kp((500.0, 360.0))
    d = P.kps[k]["descs"][0]
    P.cand(P.world((500.5, 360.0), 5.0), _flip(rng, d, 9)[None])
    P.cand(P.world((500.0, 360.5), 5.0), _flip(rng, d, 7)[None])
    P.cand(P.world((499.5, 360.0), 5.0), _flip(rng, d, 7)[None])
    # the minimum over both descriptor sets is neither's first descriptor
    a, b = _desc(rng)[0], _desc(rng)[0]
    k = P.kp((600.0, 150.0), descs=np.stack([a, b]), kfids=[40, 41])
    P.cand(P.world((600.2, 150.1), 4.0), np.stack([_desc(rng)[0], _flip(rng, b, 3)]), kfids=[2, 5])
    for _ in range(30):
        P.kp((rng.uniform(2, W - 2), rng.uniform(2, H - 2)))
        P.cand(P.world((rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(3, 12)), _desc(rng, 2))
    return P


def make_match_pairs(seed=4):
    """name -> pair, in a fixed order.  `revisit_a` / `revisit_b`: the plain case at two poses; `dense`: 65 / 130 keypoints in a
    cell; `borders`: border cells, the 10 px gate, ties; `masked`: every keypoint already matched; `no_kp` / `no_cand`: an empty
    side (the other side is not).  The default seed is one at which the checker's gate margins hold with room to spare
    (tests/test_loop_verify_ref_cpu.py asserts them); it was chosen on the checker alone."""
    rng = np.random.default_rng(seed)
    out = {}
    out["revisit_a"] = _general(rng, 1000).dict()
    out["dense"] = _dense(rng, 2000).dict()
    out["no_kp"] = dict(_general(rng, 3000, n_kp=10, n_cand=12).dict(), kps=[])
    out["borders"] = _borders(rng, 4000).dict()
    m = _general(rng, 5000, n_kp=40, n_cand=50).dict()
    for k in m["kps"]:
        k["matched"] = True
    out["masked"] = m
    out["no_cand"] = dict(_general(rng, 6000, n_kp=10, n_cand=12).dict(), cands=[])
    out["revisit_b"] = _general(rng, 7000, n_kp=130, n_cand=170, revisit_frac=0.7).dict()
    return out


# ---- the map around a loop candidate: what LoopCloser::trackLoopLocalMap walks in front of its matcher ----------------------
LC, NEWKF, MISSING = 30, 60, 25
COV_OF_LC = {10: 5, 14: 7, 15: 9, 22: 12, MISSING: 8, 29: 40, 31: 33, 45: 6, 46: 4, 50: 3}   # kfid -> score; 30 +- 15 = [15, 45]


def make_local_map_scene(seed=1):
    """a map in the dict layout of synth_loop.make_scene (host_map.LoopMap builds the C++ host map from it): the candidate
    keyframe LC = 30 with covisible keyframes inside its +- 15 window (15, 22, 29, 31, 45: both edges), outside it on both
    sides (10, 14 / 46, 50) and one that left the map (25); the new keyframe 60; and `vkplmids`, the pair list that reaches
    trackLoopLocalMap.  `roles` names the lmids by what must happen to them:
      local       3D keypoint of an in-window keyframe, map point 3D with a descriptor: offered to the matcher
      repeated    the same, seen from several in-window keyframes: looked at once
      identity    also a keypoint of the new keyframe: becomes an identity pair
      identity_in the same, but the identity pair is already in vkplmids: not appended again
      second      second element of a pair of vkplmids: leaves the local set
      gone / no_desc / not3d   in the local set, refused by the candidate filter
      only2d      2D keypoint in every in-window keyframe that sees it: never looked at
      outside     3D keypoints of keyframes outside the window or of the missing keyframe only: never looked at"""
    rng = np.random.default_rng(seed)
    inwin, outwin = [15, 22, 29, LC, 31, 45], [10, 14, 46, 50]
    kps = {k: [] for k in inwin + outwin + [NEWKF]}
    desc, roles, nxt = {}, {r: [] for r in ("local", "repeated", "identity", "identity_in", "second", "gone", "no_desc", "not3d",
                                            "only2d", "outside")}, [500]

    def lm(role, with_desc=True):
        nxt[0] += int(rng.integers(1, 4))
        roles[role].append(nxt[0])
        if with_desc:
            desc[nxt[0]] = rng.integers(0, 256, 32, dtype=np.uint8)
        return nxt[0]

    def see(kf, l, kp3d=True):
        kps[kf].append((l, tuple(rng.uniform([20, 20], [W - 20, H - 20]).astype(np.float32)), kp3d))

    for k in inwin:
        for _ in range(18):
            see(k, lm("local"))
    for _ in range(14):
        l = lm("repeated")
        for k in rng.choice(inwin, size=int(rng.integers(2, 4)), replace=False):
            see(int(k), l)
    for role, n in (("identity", 9), ("identity_in", 3)):
        for _ in range(n):
            l = lm(role)
            see(int(rng.choice(inwin)), l)
            see(NEWKF, l)
    for _ in range(34):
        see(int(rng.choice(inwin)), lm("second"))
    for _ in range(5):
        see(int(rng.choice(inwin)), lm("gone"))
        see(int(rng.choice(inwin)), lm("no_desc", with_desc=False))
        l = lm("not3d")                  # created by keyframe 10 from a 2D keypoint: the map point is not 3D
        see(10, l, kp3d=False)
        see(int(rng.choice(inwin)), l)
        l = lm("only2d")
        see(int(rng.choice(inwin)), l, kp3d=False)
        see(14, l)
    for k in outwin + [MISSING]:
        kps.setdefault(k, [])
        for _ in range(8):
            see(k, lm("outside"))
    new_own = []
    for _ in range(90):
        nxt[0] += 1
        desc[nxt[0]] = rng.integers(0, 256, 32, dtype=np.uint8)
        see(NEWKF, nxt[0], rng.random() < 0.8)
        new_own.append(nxt[0])
    vkplmids = [(int(q), int(l)) for q, l in zip(new_own, roles["second"])] + [(l, l) for l in roles["identity_in"]]
    vkplmids = [vkplmids[i] for i in rng.permutation(len(vkplmids))]
    # geometry: the pose the new keyframe really has (what a P3P on these pairs would return), a world point for every map
    # point -- in view of that pose, so that the matcher has something to refuse -- and, for 50 local map points, the place of
    # one of the new keyframe's own keypoints: the same corner under an old lmid, its descriptor a few bits apart, with a
    # second, closer descriptor from another old keyframe.  new_own[:34] are first elements of vkplmids (masked), so the
    # twins of new_own[30:34] find their keypoint taken.
    R, t = synth_ba.se3_exp(np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.1, 3)]))
    px_new = {l: np.float64(px) for l, px, _ in kps[NEWKF]}

    def backproject(px, z):
        return R @ np.array([(px[0] - K4[2]) / K4[0] * z, (px[1] - K4[3]) / K4[1] * z, z]) + t

    wpt = {l: backproject(rng.uniform([0, 0], [W, H]), rng.uniform(3, 12)) for k in kps for l, _, _ in kps[k]}
    descs, twins = {}, set()
    for q, l in zip(new_own[:34], roles["second"]):      # the incoming pairs are what a P3P kept: true correspondences
        wpt[l] = backproject(px_new[q] + rng.normal(0, 0.3, 2), rng.uniform(3, 12)) + rng.normal(0, 0.002, 3)
        twins.add((int(q), int(l)))
    for q, l in zip(new_own[30:80], roles["local"][:50]):
        wpt[l] = backproject(px_new[q] + rng.normal(0, 0.3, 2), rng.uniform(3, 12)) + rng.normal(0, 0.002, 3)
        desc[l] = _flip(rng, desc[q], int(rng.integers(8, 16)))
        descs[l] = [(int(rng.integers(0, 9)), _flip(rng, desc[q], int(rng.integers(1, 7))))]   # another old keyframe's, closer
        twins.add((int(q), int(l)))
    for k in kps:                        # keyframes hold their keypoints in no particular order
        kps[k] = [kps[k][i] for i in rng.permutation(len(kps[k]))]
    kfids = sorted(k for k in kps if k != MISSING)
    poses = {k: np.array([0.05 * k, 0, 0, 0, 0, 0, 1.0]) for k in kfids}
    dR, dt = synth_ba.se3_exp(np.array([0.2, -0.18, 0.12, 0.02, -0.025, 0.015]))     # the stored pose has drifted: 0.3 m, 2 degrees
    poses[NEWKF] = synth_ba.pose7(R @ dR, t + dt)
    # keyframe 25 is in the covisibility map of the candidate but not in the map; its keypoints exist nowhere
    out_kps = {k: dict(lmid=np.array([r[0] for r in kps[k]], np.int32), uv=np.array([r[1] for r in kps[k]], np.float32).reshape(-1, 2),
                       kp3d=np.array([r[2] for r in kps[k]], np.uint8), xyz=np.array([wpt[r[0]] for r in kps[k]]).reshape(-1, 3))
               for k in kfids}
    seen = set(int(l) for k in kfids for l in out_kps[k]["lmid"])
    return dict(K4=K4, w=W, h=H, kfids=kfids, poses=poses, kps=out_kps,
                desc={l: d for l, d in desc.items() if l in seen}, forget_lm=sorted(roles["gone"]),
                cov=[(LC, k, s) for k, s in COV_OF_LC.items()], pairs=dict(revisit=(NEWKF, LC)), vkplmids=vkplmids, roles=roles,
                Twc=synth_ba.pose7(R, t), wpt=wpt, descs=descs, true_pairs=twins, grid_kfs=[NEWKF], cell=CELL)


def track_jobs(s):
    """name -> (newkf, lckf, Twc, vkplmids): the trackLoopLocalMap calls the tests make on a make_local_map_scene map.
    `true`: the scene's pose and pair list; `empty_list`: no incoming pairs (nothing masked, every identity pair appended);
    `shifted`: the pose 4 cm off, projections a few pixels off, still inside the 10 px gate for most; `away`: the camera turned
    round, nothing projects; `other_kf`: keyframe 10 as the candidate (its window holds 10, 14, 15, 22 of the map and nothing
    of its own covisibility map but itself)"""
    T = np.asarray(s["Twc"], np.float64)
    shifted = T.copy()
    shifted[:3] += [0.04, -0.02, 0.01]
    R = synth_ba.quat_to_rot(T[3:])
    away = synth_ba.pose7(R @ np.diag([-1.0, 1.0, -1.0]), T[:3])
    return dict(true=(NEWKF, LC, T, s["vkplmids"]), empty_list=(NEWKF, LC, T, []), shifted=(NEWKF, LC, shifted, s["vkplmids"][:4]),
                away=(NEWKF, LC, away, s["vkplmids"]), other_kf=(NEWKF, 10, T, s["vkplmids"]))


def pnp_job(s, tracked):
    """the computePnP call the tests make: the pair list `tracked` that trackLoopLocalMap leaves for the job `true` (the
    incoming pairs and the revisits found by the matcher: true correspondences; the identity pairs, whose world points are
    unrelated to their pixels: outliers), with one pair whose map point is gone and one whose keypoint the new keyframe does
    not hold put in front; a start pose 3 cm and 0.5 degrees off; an outlier list that already holds an entry.
    returns (vkplmids, Twc0, voutlier_idx)"""
    pairs = [(tracked[0][0], s["roles"]["gone"][0]), (987654, tracked[-1][1])] + [tuple(p) for p in tracked]
    R0, t0 = synth_ba.quat_to_rot(np.asarray(s["Twc"][3:])), np.asarray(s["Twc"][:3])
    dR, _ = synth_ba.se3_exp(np.array([0, 0, 0, 0.005, -0.006, 0.004]))
    return pairs, synth_ba.pose7(R0 @ dR, t0 + [0.02, -0.02, 0.01]), [1]


NRANSAC_ITER, FRANSAC_ERR = 100, 3.0


def verify_pairs(s):
    """name -> (newkf, lckf, vkplmids): the candidate pairs that reach the 2D-3D half of processLoopCandidate (:238-300) on a
    make_local_map_scene map, named by where they must end:
      accept    the scene's list (34 true pairs, 3 identity pairs unrelated to the loop pose): P3P, ~46 new matches, PnP >= 30
      p3p_fail  world points unrelated to the pixels: no model with 5 inliers
      gone      accept's list with five pairs whose map point is gone mixed in (the vbadidx erasure); still accepted
      no_new    keyframe 50 as the candidate: its local map is its own 8 unrelated points, nothing new is matched
      pnp_few   keyframe 29 as the candidate with a short list: new matches, but fewer than 30 inliers after PnP
      lt4       a hand-made list of 3 pairs
      outwin    keyframe 10 as the candidate: every keyframe that could support the loop lies outside its +- 15 window"""
    ro, base = s["roles"], list(s["vkplmids"])
    own = [q for q, l in base if q != l]
    gone = list(base)
    for i, l in enumerate(ro["gone"]):
        gone.insert(3 + 5 * i, (own[i], l))
    true = [p for p in base if p[0] != p[1]]
    return dict(accept=(NEWKF, LC, base), p3p_fail=(NEWKF, LC, [(q, l) for q, l in zip(own, ro["outside"][:20])]),
                gone=(NEWKF, LC, gone), no_new=(NEWKF, 50, base), pnp_few=(NEWKF, 29, true[:8]), lt4=(NEWKF, LC, true[:3]),
                outwin=(NEWKF, 10, base))
