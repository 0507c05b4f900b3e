"""Seeded inputs of the batched local-map matcher (ov2_match_to_map_batch = Mapper::matchToMap, src/mapper.cpp:576-774, for B
frames): a new keyframe whose keypoints carry map points, and the local map it is re-matched against.

Frames are dicts as mapper.MatchBatchInput takes them -- Twc, kps [px, descs, kfids, kf_px], cands [wpt, descs, kfids], kf_Twc
-- plus nb3dkps (Frame::nb3dkps_).  They are built the way tests/test_match.py builds its scene: planted re-observations of a
keypoint's landmark from other keyframes, co-observed pairs, candidates behind the camera, candidates without descriptors and
unrelated points.  The shapes are the smallest that still reach every path of the kernel (120 keypoints x 300 candidates x 12
keyframes unless said otherwise): they are not EuRoC sizes; timing_frame makes one of those.  Every planted effect is listed
at its frame below and counted on the checker by tests/test_match_batch_cpu.py."""
import numpy as np

from . import mapper, synth, synth_ba

K4 = np.array([458.654, 457.296, 367.215, 248.375])
W, H, CELL = 752, 480, 35
CELL_DENSE = 376            # a 2 x 2 grid: the `dense` frame then has cells of more than 64 keypoints
CAMERA = (K4, W, H, CELL)
FMAXPROJERR, FDISTRATIO = 2.0, 0.2
RADTAN = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)   # EuRoC cam0, for the lens-model case
NB3D = 120


def _proj(T, X):
    Rk, tk = synth_ba.quat_to_rot(T[3:]), T[:3]
    pc = (X - tk) @ Rk
    return np.float32([K4[0] * pc[0] / pc[2] + K4[2], K4[1] * pc[1] / pc[2] + K4[3]])


def _flip(rng, d, nbits):
    d = d.copy()
    for f in rng.integers(0, 256, size=nbits):
        d[f >> 3] ^= np.uint8(1 << (f & 7))
    return d


def _frame(seed, n_kp=120, n_cand=300, n_kf=12, nb3dkps=NB3D, sideways=0, px=None, Twc=None):
    """the plain frame.  sideways: that many of the planted re-observations are pushed 3 px along x in the image, outside
    the 2 px gate and inside the doubled one"""
    rng = np.random.default_rng(seed)
    kf_Twc = np.array([synth_ba.pose7(synth_ba.se3_exp(np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)]))[0],
                                      rng.normal(0, 0.3, 3)) for _ in range(n_kf)])
    if Twc is not None:
        kf_Twc[-1] = Twc
    Twc = kf_Twc[-1].copy()
    R, t = synth_ba.quat_to_rot(Twc[3:]), Twc[:3]
    if px is None:
        px = synth.grid_keypoints(n_kp, seed=seed + 1)
    n_kp = len(px)
    z = rng.uniform(3, 12, n_kp)

    def world(p, zz):
        return R @ np.array([(p[0] - K4[2]) / K4[0] * zz, (p[1] - K4[3]) / K4[1] * zz, zz]) + t
    wpts = np.array([world(px[i], z[i]) for i in range(n_kp)])
    kps, cands = [], []
    for i in range(n_kp):
        kfids = sorted(rng.choice(n_kf - 2, size=rng.integers(1, 4), replace=False).tolist())
        descs = rng.integers(0, 256, (len(kfids), 32), dtype=np.uint8) if rng.uniform() > 0.05 else np.zeros((0, 32), np.uint8)
        kf_px = np.array([_proj(kf_Twc[k], wpts[i]) + rng.normal(0, 0.4, 2) for k in kfids], np.float32).reshape(-1, 2)
        kps.append(dict(px=px[i], descs=descs, kfids=kfids, kf_px=kf_px))
    pushed = 0
    for c in range(n_cand):
        u = rng.uniform()
        i = int(rng.integers(n_kp))
        kd = kps[i]["descs"]
        if u < 0.5 and len(kd):          # a re-observation of keypoint i's landmark from other keyframes
            d = _flip(rng, kd[rng.integers(len(kd))], int(rng.integers(0, 30)))
            kf = sorted(set(range(n_kf)) - set(kps[i]["kfids"]))
            kfids = sorted(rng.choice(kf, size=2, replace=False).tolist())
            if pushed < sideways:
                w = world(np.float64(px[i]) + [3.0, 0.0], z[i])
                pushed += 1
            else:
                w = wpts[i] + rng.normal(0, 0.004, 3)
            cands.append(dict(wpt=w, descs=np.stack([d, rng.integers(0, 256, 32, dtype=np.uint8)]), kfids=kfids))
        elif u < 0.6 and len(kd):        # same landmark but co-observed in one keyframe: never a candidate
            cands.append(dict(wpt=wpts[i], descs=kd[:1].copy(), kfids=sorted({kps[i]["kfids"][0], n_kf - 1})))
        elif u < 0.7:                    # behind the camera / outside the field of view
            cands.append(dict(wpt=t + R @ np.array([rng.normal(), rng.normal(), -rng.uniform(0.5, 3)]),
                              descs=rng.integers(0, 256, (1, 32), dtype=np.uint8), kfids=[0]))
        elif u < 0.75:                   # no descriptor
            cands.append(dict(wpt=wpts[i], descs=np.zeros((0, 32), np.uint8), kfids=[0]))
        else:                            # unrelated point somewhere in view
            cands.append(dict(wpt=world((rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(3, 12)),
                              descs=rng.integers(0, 256, (2, 32), dtype=np.uint8), kfids=[int(rng.integers(n_kf))]))
    return dict(Twc=Twc, kps=kps, cands=cands, kf_Twc=kf_Twc, nb3dkps=nb3dkps)


def _on_zero(f, c):
    """(v, z): a camera coordinate and a depth for which the pinhole projection f * (v * (1 / z)) + c, evaluated in double as
    the kernel does, is the smallest value >= 0 that a double reaches: exactly 0 where one does (one ulp of v moves the product
    by about two of its own), under 1e-13 px otherwise"""
    z = 4.0          # the depth _borders uses
    vs = [-(c / f) * z]
    for _ in range(4):
        vs = [np.nextafter(vs[0], -np.inf)] + vs + [np.nextafter(vs[-1], np.inf)]
    p, v = min((f * (v * (1.0 / z)) + c, v) for v in vs if f * (v * (1.0 / z)) + c >= 0.0)
    assert p < 1e-13
    return float(v), z


EDGE = [(0.75, 249.0), (366.0, 0.75), (3.5, 240.5), (20.0, 260.5), (300.5, 12.0), (400.0, 3.5), (738.5, 250.0), (741.0, 244.0),
        (330.0, H - 1.5), (400.0, H - 2.5), (360.0, 34.5), (34.5, 248.0), (500.0, 470.0)]
N_EDGE = len(EDGE)          # the first keypoints of the `borders` frame; candidates land on x = 0 beside [0], on y = 0 beside [1]


def _borders(seed):
    """keypoints in the first and last rows and columns of cells (the 2 x 2 walk then leaves the grid on one side), each with a
    planted re-observation; and, at the identity pose so that world = camera coordinates, candidates that project onto x = 0 and
    onto y = 0 with a keypoint next to them.  They sit near the image axes: Mapper's view-angle gate (:586-598, :640-645)
    refuses what projects into the image corners, and past x = 743 in the middle rows"""
    px = np.concatenate([np.float32(EDGE), synth.grid_keypoints(120 - N_EDGE, seed=seed + 1)])
    f = _frame(seed, n_cand=280, px=px, Twc=np.array([0, 0, 0, 0, 0, 0, 1.0]))
    rng = np.random.default_rng(seed + 2)
    n_kf = len(f["kf_Twc"])
    extra = []
    for i in range(N_EDGE):
        k = f["kps"][i]
        if not len(k["descs"]):
            k["descs"] = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        z = 4.0
        w = np.array([(px[i, 0] - K4[2]) / K4[0] * z, (px[i, 1] - K4[3]) / K4[1] * z, z])
        if i < 2:          # onto x = 0 beside keypoint 0, onto y = 0 beside keypoint 1
            w[i], _ = _on_zero(K4[i], K4[2 + i])
        kf = sorted(set(range(n_kf)) - set(k["kfids"]))[:2]
        k["kf_px"] = np.array([_proj(f["kf_Twc"][q], w) for q in k["kfids"]], np.float32).reshape(-1, 2)
        extra.append(dict(wpt=w, descs=np.stack([_flip(rng, k["descs"][0], 5)]), kfids=kf))
    f["cands"] = f["cands"][:140] + extra + f["cands"][140:]
    return f


def _short_kf(seed):
    """keyframe lists that name ids past the frame's own pose table: the table is cut to 8 poses while the lists go up to 9, so
    some keypoints lose a part of their mean-reprojection sum and some all of it (0 / 0: the gate lets them through)"""
    f = _frame(seed)
    f["kf_Twc"] = f["kf_Twc"][:8].copy()
    return f


def make_frames(seed=1):
    """name -> frame, in a fixed order.  `plain_a` / `plain_b`: the plain case at two seeds; `few3d`: nb3dkps = 29 with 60
    planted candidates 3 px sideways, which only the doubled gate lets in; `no_kp` / `no_cand`: an empty side (the other side is
    not); `borders`: border cells and projections onto x = 0 / y = 0; `short_kf`: keyframe ids past the pose table; `dense`:
    300 keypoints x 600 candidates, for a call with cell = CELL_DENSE.  The default seed was chosen on the checker alone."""
    out = {}
    out["plain_a"] = _frame(100 * seed + 1)
    out["few3d"] = _frame(100 * seed + 2, nb3dkps=29, sideways=60)
    out["no_kp"] = dict(_frame(100 * seed + 3, n_kp=10, n_cand=14), kps=[])
    out["borders"] = _borders(100 * seed + 4)
    out["no_cand"] = dict(_frame(100 * seed + 5, n_kp=10, n_cand=14), cands=[])
    out["short_kf"] = _short_kf(100 * seed + 6)
    out["dense"] = _frame(100 * seed + 7, n_kp=300, n_cand=600)
    out["plain_b"] = _frame(100 * seed + 8)
    return out


def batches(frames):
    """name -> frame names: the compositions the tests run in one call (reversed, repeated, the empty frames first, in the
    middle and last; few3d always between two frames whose gate is not doubled)"""
    n = list(frames)
    return dict(all=n, reversed=n[::-1] + ["dense", "no_cand", "no_kp", "dense"], empty_first=["no_kp", "no_cand", "plain_a", "few3d", "plain_b"],
                empty_middle=["plain_a", "few3d", "no_cand", "no_kp", "plain_b", "short_kf"], empty_last=["borders", "plain_a", "few3d", "plain_b", "no_cand", "no_kp"])


def single_input(f, K=K4, img_w=W, img_h=H, cell=CELL, nb3dkps=None, cam=None):
    """the ov2_match_to_map input of one frame"""
    return mapper.MatchInput(f["Twc"], K, img_w, img_h, cell, f["nb3dkps"] if nb3dkps is None else nb3dkps, f["kps"], f["cands"],
                             f["kf_Twc"], cam=cam)


def batch_input(frames, K=K4, img_w=W, img_h=H, cell=CELL, cam=None):
    """the ov2_match_to_map_batch input of a list of frames"""
    return mapper.MatchBatchInput(frames, K, img_w, img_h, cell, [f["nb3dkps"] for f in frames], cam=cam)


def timing_frame(seed, n_kp=300, n_cand=2500, n_kf=50):
    """a EuRoC-sized frame for scripts/match_time.py: about 300 keypoints, a local map of 2000-3000 candidates, 50 keyframes"""
    return _frame(seed, n_kp=n_kp, n_cand=n_cand, n_kf=n_kf)


# ---- the host stage: B maps, one new keyframe and one local set each -----------------------------------------------------

def local_map_scenes(seeds=(1, 2, 3)):
    """synth_revisit.make_local_map_scene maps for host_map.match_local_maps: the new keyframe's STORED pose is set to the pose
    it really has (Mapper::matchToMap projects with the frame's own pose; the loop closer's scenes store a drifted one), and
    `local` lists the lmids of the candidate keyframe's neighbourhood in a seeded order: the planted twins of the new
    keyframe's keypoints (roles local[:50]), identity points the frame already observes, points that are gone, not 3D or
    without descriptor, and unrelated ones"""
    from . import synth_revisit as SR
    out = []
    for seed in seeds:
        s = SR.make_local_map_scene(seed)
        s["poses"][SR.NEWKF] = np.asarray(s["Twc"], np.float64).copy()
        ro = s["roles"]
        local = [int(l) for r in ("local", "repeated", "identity", "identity_in", "second", "gone", "no_desc", "not3d", "only2d")
                 for l in ro[r]]
        rng = np.random.default_rng(1000 + seed)
        s["local"] = [local[i] for i in rng.permutation(len(local))]
        out.append(s)
    return out
