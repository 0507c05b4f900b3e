"""numpy restatement of the two mono host stages that use the refined 5-point model, built on the pieces of
tests/epipolar_ref.py (bearings, pair order, parallax sum, RANSAC) and tests/relpose_ref.py (the refinement):
the mono do_optimize branch of VisualFrontEnd::epipolar2d2dFiltering (reference src/visual_front_end.cpp:446-608) and
VisualFrontEnd::checkReadyForInit (:855-984).  Frames are {lmid: (undistorted pixel (2,) float32, is3d)}, poses are
[t, qx qy qz qw] camera-to-world, as the C++ mirror stores them."""
import math

import numpy as np

import epipolar_ref as ER
import relpose_ref as RR

NREFINE = 10     # MultiViewGeometry::kRefine5ptIters


# ---- SE3 of the C++ mirror ----------------------------------------------------------------------------------------------
def se3_R(T):
    return np.array(ER.se3_rotation(T[3:])).reshape(3, 3)


def _quat_of(R):
    """rot_to_quat of SE3::fromRt: the branches of relpose_ref.rot_to_quat, not normalised"""
    R = [float(v) for v in np.asarray(R).ravel()]
    t = R[0] + R[4] + R[8]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return [(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, 0.25 * s]
    if R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(1.0 + R[0] - R[4] - R[8]) * 2
        return [0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s]
    if R[4] > R[8]:
        s = math.sqrt(1.0 + R[4] - R[0] - R[8]) * 2
        return [(R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s, (R[2] - R[6]) / s]
    s = math.sqrt(1.0 + R[8] - R[0] - R[4]) * 2
    return [(R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s, (R[3] - R[1]) / s]


def se3_from_Rt(R, t):
    return np.array(list(t) + _quat_of(R))


def se3_inv(T):
    R = se3_R(T)
    n = math.sqrt(float((T[3:] * T[3:]).sum()))
    return np.concatenate([-(R.T @ T[:3]), [-T[3] / n, -T[4] / n, -T[5] / n, T[6] / n]])


def se3_mul(A, B):
    Ra = se3_R(A)
    return se3_from_Rt(Ra @ se3_R(B), Ra @ B[:3] + A[:3])


# ---- the shared front: pairs in ascending lmid order -------------------------------------------------------------------
def _pairs(kf, cur, K):
    ids, bkf, bcur = [], [], []
    for lmid in sorted(cur):
        if lmid not in kf:
            continue
        ids.append(lmid)
        bkf.append(ER.bearing(kf[lmid][0], K))
        bcur.append(ER.bearing(cur[lmid][0], K))
    return ids, np.array(bkf).reshape(-1, 3), np.array(bcur).reshape(-1, 3)


def ransac_then_refine(bkf, bcur, K, nmaxiter, errth, seed):
    """compute5ptEssentialMatrix with do_optimize: (epipolar_ref.epipolar_filter result, R (9,), t (3,), refinement)"""
    e = ER.epipolar_filter(bkf, bcur, K, nmaxiter, errth, seed)
    if e["status"] < 1:
        return e, None, None, None
    r = RR.refine(bkf, bcur, K, e["R"], e["t"], NREFINE, e["outlier"])
    return e, r["R"], r["t"], r


def mono_epipolar2d2d(kf, cur, K, T_kf, T_cur, nkfs, nmaxiter, errth, seed):
    """VisualFrontEnd::epipolar2d2dFiltering with mono_ set.  returns dict(status (-1: returned before the RANSAC), removed
    (ascending), do_optimize, Twc (the current frame's pose after the stage), refine (the refinement's result or None))"""
    out = dict(status=-1, removed=[], do_optimize=0, Twc=np.array(T_cur, np.float64), refine=None)
    Rkfcur = (se3_R(se3_inv(T_kf)) @ se3_R(T_cur)).ravel()
    # steps 1-5 (the tests before the RANSAC, the float parallax sum) are those of the stereo form with stereo = False
    pre_removed, pre_status = ER.epipolar2d2d(kf, cur, K, Rkfcur, False, 0, errth, seed)   # nmaxiter 0: only the early returns matter
    if pre_status == -1:
        return out
    nb3d = sum(1 for v in cur.values() if v[1])
    do_opt = nkfs > 2 and nb3d < 30                                           # :537-544
    out["do_optimize"] = int(do_opt)
    ids, bkf, bcur = _pairs(kf, cur, K)
    e = ER.epipolar_filter(bkf, bcur, K, nmaxiter, errth, seed)
    out["status"] = e["status"]
    R, t = e["R"], e["t"]
    if do_opt and e["status"] >= 1:
        out["refine"] = RR.refine(bkf, bcur, K, R, t, NREFINE, e["outlier"])
        R, t = out["refine"]["R"], out["refine"]["t"]
    if e["status"] < 2:
        return out
    out["removed"] = sorted(ids[i] for i in np.flatnonzero(e["outlier"]))
    if do_opt and nkfs > 2:                                                   # :594-608
        Tkfcur = se3_mul(se3_inv(T_kf), np.asarray(T_cur, np.float64))
        scale = math.sqrt(float((Tkfcur[:3] * Tkfcur[:3]).sum()))
        tn = t / math.sqrt(float((t * t).sum()))
        out["Twc"] = se3_mul(np.asarray(T_kf, np.float64), se3_from_Rt(R, scale * tn))
    return out


def _median_parallax(kf, cur):
    """computeParallax(kfid, do_unrot = false): the median (element size / 2 of the ordered set) of |unpx - kf unpx|"""
    f32 = np.float32
    vals = set()
    for lmid, (px, _) in cur.items():
        if lmid not in kf:
            continue
        dx, dy = f32(f32(px[0]) - f32(kf[lmid][0][0])), f32(f32(px[1]) - f32(kf[lmid][0][1]))
        vals.add(f32(math.sqrt(float(dx) * float(dx) + float(dy) * float(dy))))
    if not vals:
        return 0.0
    return float(sorted(vals)[len(vals) // 2])


def check_ready_for_init(kf, cur, K, T_kf, T_cur, finit_parallax, nmaxiter, errth, seed):
    """VisualFrontEnd::checkReadyForInit.  returns dict(ready, removed (ascending), Twc, pairs, refine, ransac)"""
    f32 = np.float32
    out = dict(ready=False, removed=[], Twc=np.array(T_cur, np.float64), pairs=0, refine=None, ransac=None)
    fin = float(f32(finit_parallax))
    if not _median_parallax(kf, cur) > fin:                                   # :857-861
        return out
    if len(cur) < 8:                                                          # :873
        return out
    Rkfcur = (se3_R(se3_inv(T_kf)) @ se3_R(T_cur)).ravel()
    ids, bkf, bcur = _pairs(kf, cur, K)
    avg = f32(0.)
    for lmid, b in zip(ids, bcur):                                            # :893-915
        r = [Rkfcur[3 * i] * b[0] + Rkfcur[3 * i + 1] * b[1] + Rkfcur[3 * i + 2] * b[2] for i in range(3)]
        ux, uy = K[0] * r[0] + K[2] * r[2], K[1] * r[1] + K[3] * r[2]         # K * rotbv, then / z
        dx, dy = f32(f32(ux / r[2]) - f32(kf[lmid][0][0])), f32(f32(uy / r[2]) - f32(kf[lmid][0][1]))
        avg = f32(float(avg) + math.sqrt(float(dx) * float(dx) + float(dy) * float(dy)))
    out["pairs"] = len(ids)
    if len(ids) < 8:                                                          # :917
        return out
    avg = f32(avg / f32(len(ids)))                                            # :923
    if float(avg) < fin:                                                      # :925
        return out
    Kf = np.array([float(f32(K[0])), float(f32(K[1])), 0., 0.])               # fx_, fy_ pass through float parameters
    e, R, t, r = ransac_then_refine(bkf, bcur, Kf, nmaxiter, errth, seed)
    out["ransac"], out["refine"] = e, r
    if e["status"] < 1:                                                       # :956
        return out
    out["removed"] = sorted(ids[i] for i in np.flatnonzero(e["outlier"]))     # :962-965
    tn = t / math.sqrt(float((t * t).sum()))
    out["Twc"] = se3_from_Rt(R, tn * 0.25)                                    # :968-973
    out["ready"] = True
    return out
