"""numpy f64 restatement of the P3P stage of computePose (csrc/p3p.hip), the checker of the GPU tests.

The rules are those of MultiViewGeometry::p3pRansac -> opengvP3PLMeds / opengvP3PRansac (reference
src/multi_view_geometry.cpp:144-343) and OpenGV's Lmeds / Ransac over AbsolutePoseSacProblem (KNEIP), restated from
OpenGV's published source, with this project's sampler (include/ov2slam_hip.h, ov2_p3p_ransac_batch).  The P3P solver
here is deliberately another method than the kernel's Kneip parametrisation: Grunert's quartic in the depth ratio
v = s3 / s1 (Haralick et al., IJCV 13(3), 1994) through np.roots, and the pose from a three-point Procrustes alignment
(SVD).  Distance, penalty, sampler and loops use the kernel's operation order, so that integer outcomes agree exactly."""
import math

import numpy as np

from epipolar_ref import EPS, epi_hash

DBL_MAX = np.finfo(np.float64).max


def draw(seed, d, n):
    """the 4 distinct indices of draw d, n >= 4: the stream of the epipolar stage's sampler, cut after 4 (redraw on a
    duplicate; after 256 attempts the smallest unused index)"""
    idx, j = [], 0
    for _ in range(4):
        v = -1
        while v < 0 and j < 256:
            c = epi_hash(seed, d, j, n)
            j += 1
            if c not in idx:
                v = c
        if v < 0:
            v = min(c for c in range(n) if c not in idx)
        idx.append(v)
    return idx


def threshold(errth, fx, fy):
    """1 - cos(atan(errth / focal)): focal = (fx + fy) / 2 and the quotient in float (src/multi_view_geometry.cpp:298-302)"""
    focal = np.float32(np.float32(fx) + np.float32(fy))
    focal = np.float32(np.float64(focal) / 2.)
    q = np.float32(np.float32(errth) / focal)
    return 1.0 - math.cos(math.atan(float(q)))


def score(R, t, f, X):
    """1 - f . p / |p|, p = R^T (X - t), unclamped, the kernel's operation order; R (9,) row-major; vectorised"""
    f, X = np.atleast_2d(f), np.atleast_2d(X)
    with np.errstate(all="ignore"):
        v0, v1, v2 = X[:, 0] - t[0], X[:, 1] - t[1], X[:, 2] - t[2]
        p0 = R[0] * v0 + R[3] * v1 + R[6] * v2
        p1 = R[1] * v0 + R[4] * v1 + R[7] * v2
        p2 = R[2] * v0 + R[5] * v1 + R[8] * v2
        n = np.sqrt(p0 * p0 + p1 * p1 + p2 * p2)
        return 1.0 - (f[:, 0] * (p0 / n) + f[:, 1] * (p1 / n) + f[:, 2] * (p2 / n))


def dist(R, t, f, X):
    """the distance the loops use: clamped below at 0; a non-finite one counts as +infinity"""
    d = score(R, t, f, X)
    d = np.where(np.isfinite(d), d, np.inf)
    return np.where(d < 0., 0., d)


# ---- Grunert's P3P -----------------------------------------------------------------------------------------------------
def p3p_grunert(f, X, return_roots=False):
    """all [R_wc (3,3), t_wc (3,)] with s_i f_i = R^T (X_i - t), s_i > 0, for the three bearings f (3,3) and points X (3,3)"""
    f, X = np.asarray(f, np.float64), np.asarray(X, np.float64)
    sols, roots = [], np.zeros(0, complex)
    out = lambda: (sols, roots) if return_roots else sols
    if not (np.isfinite(f).all() and np.isfinite(X).all()):
        return out()
    a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
    if not (np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0])) > 0.) or b2 == 0.:
        return out()
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    k1, k2 = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (k1 - 1) ** 2 - 4 * c2 / b2 * ca ** 2
    A3 = 4 * (k1 * (1 - k1) * cb - (1 - k2) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb)
    A2 = 2 * (k1 ** 2 - 1 + 2 * k1 ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * k2 * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2)
    A1 = 4 * (-k1 * (1 + k1) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - k2) * ca * cg)
    A0 = (1 + k1) ** 2 - 4 * a2 / b2 * cg ** 2
    co = np.array([A4, A3, A2, A1, A0])
    if not np.isfinite(co).all() or not np.any(co[:-1] != 0):
        return out()
    roots = np.roots(co)
    mX = X.mean(0)
    for v in roots:
        if abs(v.imag) > 1e-7 * (1 + abs(v)) or not v.real > 0:
            continue
        v = v.real
        with np.errstate(all="ignore"):
            u = ((-1 + k1) * v * v - 2 * k1 * cb * v + 1 + k1) / (2 * (cg - v * ca))
            s1 = math.sqrt(b2 / (1 + v * v - 2 * v * cb)) if 1 + v * v - 2 * v * cb > 0 else np.nan
        s = np.array([s1, u * s1, v * s1])
        if not np.isfinite(s).all():
            continue
        C = np.array([[0, 1, cg], [0, 2, cb], [1, 2, ca]], object)
        E = [c2, b2, a2]
        best, bg = s.copy(), np.inf
        for _ in range(6):      # Newton on the three distance constraints
            g = np.array([s[i] ** 2 + s[j] ** 2 - 2 * s[i] * s[j] * c - e for (i, j, c), e in zip(C, E)])
            gn = np.abs(g).sum()
            if not gn < bg:
                break
            best, bg = s.copy(), gn
            J = np.zeros((3, 3))
            for r, (i, j, c) in enumerate(C):
                J[r, i], J[r, j] = 2 * (s[i] - s[j] * c), 2 * (s[j] - s[i] * c)
            try:
                s = s - np.linalg.solve(J, g)
            except np.linalg.LinAlgError:
                break
        s = best
        if not (s > 0).all():
            continue
        A = s[:, None] * f
        mA = A.mean(0)
        U, _, Vt = np.linalg.svd((X - mX).T @ (A - mA))
        D = np.diag([1., 1., np.linalg.det(U @ Vt)])
        R = U @ D @ Vt
        t = mX - R @ mA
        p = (X - t) @ R
        if not np.abs(p / np.linalg.norm(p, axis=1, keepdims=True) - f).max() < 1e-10:
            continue
        if any(np.abs(s - q).max() <= 1e-9 * np.abs(s).max() for q, _, _ in sols):
            continue
        sols.append((s, R, t))
    sols = [(R, t) for _, R, t in sols]
    return out()


def model(f4, X4, return_gap=False):
    """OpenGV computeModelCoefficients (KNEIP): P3P on the first three, the 4th picks the lowest score.
    (ok, R (9,), t (3,)[, relative gap of the two lowest scores])"""
    best, bm, scs = np.inf, None, []
    for R, t in p3p_grunert(f4[:3], X4[:3]):
        sc = score(R.ravel(), t, f4[3], X4[3])[0]
        scs.append(sc)
        if sc < best:
            best, bm = sc, (R.ravel().copy(), t.copy())
    gap = np.inf
    if len(scs) >= 2:
        a, b = sorted(scs)[:2]
        gap = (b - a) / max(abs(b), 1e-300) if np.isfinite(b) else np.inf
    if bm is None:
        return (False, None, None, gap) if return_gap else (False, None, None)
    return (True, bm[0], bm[1], gap) if return_gap else (True, bm[0], bm[1])


def penalty(d):
    """OpenGV Lmeds: the median of the sorted distances, on their square roots"""
    d = np.sort(d)
    n = len(d)
    mid = n // 2
    with np.errstate(all="ignore"):
        return (math.sqrt(d[mid - 1]) + math.sqrt(d[mid])) / 2 if n % 2 == 0 else math.sqrt(d[mid])


# ---- the loops ---------------------------------------------------------------------------------------------------------
def lmeds(bv, X, nmaxiter, seed):
    """OpenGV Lmeds::computeModel: (best (R, t) or None, info [counted, skipped, chosen draw], gaps dict)"""
    n = len(bv)
    counted, skipped, d, best, best_d, bm = 0, 0, 0, DBL_MAX, -1, None
    pen_gap, sc_gap, seen, pens, models = np.inf, np.inf, {}, {}, {}
    if n >= 4:
        while counted < nmaxiter and skipped < 10 * nmaxiter:
            idx = draw(seed, d, n)
            ok, R, t, g = model(bv[idx], X[idx], True)
            if not ok:
                skipped += 1
                d += 1
                continue
            sc_gap = min(sc_gap, g)
            pen = penalty(dist(R, t, bv, X))
            pens[d] = pen
            models[d] = (R, t)
            if tuple(idx) not in seen and best_d >= 0 and np.isfinite(pen):
                pen_gap = min(pen_gap, abs(pen - best) / max(pen, best) if max(pen, best) > 0 else 0.)
            seen[tuple(idx)] = d
            if pen < best:
                best, best_d, bm = pen, d, (R, t)
            counted += 1
            d += 1
    return bm, [counted, skipped, best_d], dict(penalty=pen_gap, score=sc_gap, draws=seen, pens=pens, models=models)


def ransac(bv, X, nmaxiter, th, seed):
    """OpenGV Ransac::computeModel, probability 0.99, sample size 4: (best (R, t) or None, info [iterations, skipped, d])"""
    n = len(bv)
    it, skipped, k, best, best_d, bm, d = 0, 0, 1.0, -(2 ** 31 - 1), -1, None, 0
    sc_gap, seen = np.inf, {}
    if n >= 4:
        while it < k and skipped < 10 * nmaxiter:
            idx = draw(seed, d, n)
            ok, R, t, g = model(bv[idx], X[idx], True)
            if not ok:
                skipped += 1
                d += 1
                continue
            sc_gap = min(sc_gap, g)
            seen[tuple(idx)] = d
            cnt = int((dist(R, t, bv, X) < th).sum())
            if cnt > best:
                best, best_d, bm = cnt, d, (R, t)
                w = best / n
                p = min(max(EPS, 1.0 - w ** 4.0), 1.0 - EPS)
                k = math.log(1.0 - 0.99) / math.log(p)
            it += 1
            d += 1
            if it > nmaxiter:
                break
    return bm, [it, skipped, best_d], dict(penalty=np.inf, score=sc_gap, draws=seen, pens={}, models={})


def rot_to_quat(R):
    """the C++ mirror's rot_to_quat (SE3::fromRt): R (9,) row-major -> qx qy qz qw"""
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


def classify(bv, X, th, use_lmeds, bm):
    """the return rule under the model bm = (R, t) or None: (status, Twc or None, outlier mask, inlier count)"""
    n = len(bv)
    out = np.zeros(n, bool)
    if bm is None:
        return 0, None, out, 0
    R, t = bm
    d = dist(R, t, bv, X)
    inl = d <= th if use_lmeds else d < th
    ninl = int(inl.sum())
    R3 = R.reshape(3, 3)
    orth = np.linalg.norm(R3 @ R3.T - np.eye(3)) < 1e-10          # Sophus::isOrthogonal
    if ninl >= 5 and orth:
        return 1, np.array(list(t) + rot_to_quat(R)), ~inl, ninl
    return 0, None, out, ninl


def p3p_ransac(bv, wpts, K, nmaxiter, errth, use_lmeds, seed):
    """one frame of ov2_p3p_ransac_batch: dict(status, Twc (7,) or None, R, t, outlier (n,) bool, info [counted, skipped,
    chosen draw, inliers], th, gaps).  gaps["models"] / ["pens"] hold every counted LMedS draw's model and penalty, so that
    a test can name the draws tied with the winner and classify under any of them (tied_results)"""
    bv, X = np.asarray(bv, np.float64).reshape(-1, 3), np.asarray(wpts, np.float64).reshape(-1, 3)
    th = threshold(errth, K[0], K[1])
    bm, info, gaps = lmeds(bv, X, nmaxiter, seed) if use_lmeds else ransac(bv, X, nmaxiter, th, seed)
    status, Twc, out, ninl = classify(bv, X, th, use_lmeds, bm)
    R, t = bm if bm is not None else (None, None)
    return dict(status=status, Twc=Twc, R=R, t=t, outlier=out, info=info + [ninl], th=th, gaps=gaps)


def tied_results(bv, wpts, e, rel, abs_tol=0.):
    """{draw: (status, Twc, outlier, inliers)} for the LMedS draws of result e whose penalty is within rel (relative)
    + abs_tol of the winner's: the results a kernel may legitimately return when rounding breaks the tie the other way"""
    bv, X = np.asarray(bv, np.float64).reshape(-1, 3), np.asarray(wpts, np.float64).reshape(-1, 3)
    pens, best = e["gaps"]["pens"], e["info"][2]
    if best < 0:
        return {}
    return {d: classify(bv, X, e["th"], True, e["gaps"]["models"][d]) for d, p in pens.items()
            if abs(p - pens[best]) <= rel * pens[best] + abs_tol}


# ---- VisualFrontEnd::computePose (src/visual_front_end.cpp:659-851) ---------------------------------------------------
SEED_MIX = 0xD1B54A32D192ED03      # OV2_P3P_SEED_MIX of the C++ mirror


def compute_pose(pnp_solve, kps, K, Twc0, bp3preq, dop3p, mono, nransac_iter, errth, seed):
    """the reference function on one frame.  kps: {lmid: (undistorted pixel (2,) float32, world point (3,))} -- the 3D keypoints
    whose map point exists; pnp_solve: the CPU oracle's ceresPnP; seed: the stage's sampler seed before the mix (bdo_random
    off).  3D keypoints in ascending lmid order.  returns dict(removed ids ascending, reset, p3p_req, Twc, p3p: the P3P
    result or None)"""
    from epipolar_ref import bearing
    ids = sorted(kps)
    Twc = np.array(Twc0, np.float64)
    res = dict(removed=[], reset=False, p3p_req=bool(bp3preq), Twc=Twc, p3p=None)
    if len(ids) < 4:                                                      # :667
        return res
    bdop3p = bool(bp3preq or dop3p)                                       # :688
    unpx = [np.asarray(kps[i][0], np.float32).astype(np.float64) for i in ids]
    wpts = [np.asarray(kps[i][1], np.float64) for i in ids]
    removed = []
    if bdop3p:                                                            # :718-782
        bvs = np.array([bearing(kps[i][0], K) for i in ids])
        Kf = [float(np.float32(K[0])), float(np.float32(K[1])), 0., 0.]
        r = p3p_ransac(bvs, np.array(wpts), Kf, nransac_iter, errth, True, (seed ^ SEED_MIX) & ((1 << 64) - 1))
        res["p3p"] = r
        nbinliers = len(ids) - int(r["outlier"].sum())
        if r["status"] != 1 or nbinliers < 5 or not np.isfinite(r["Twc"][:3]).all():   # :750-761 -> resetFrame()
            res.update(removed=list(ids), reset=True)
            return res
        Twc = r["Twc"].copy()
        res["Twc"] = Twc                                                  # :766
        keep = ~r["outlier"]
        removed = [i for i, k in zip(ids, keep) if not k]                 # :769-778
        ids = [i for i, k in zip(ids, keep) if k]
        unpx = [u for u, k in zip(unpx, keep) if k]
        wpts = [w for w, k in zip(wpts, keep) if k]
    Kf = [float(np.float32(v)) for v in K]
    ok, T, out, _ = pnp_solve(np.array(unpx).reshape(-1, 2), np.array(wpts).reshape(-1, 3), Kf, Twc)   # :790-801
    nout = int(out.sum())
    if not ok or len(ids) - nout < 5 or nout > 0.5 * len(ids) or not np.isfinite(T[:3]).all():        # :809-832
        if not bdop3p:
            res["p3p_req"] = True
        elif mono:
            res.update(removed=sorted(removed + ids), reset=True)
            return res
        res["removed"] = sorted(removed)
        return res
    res.update(Twc=T, p3p_req=False, removed=sorted(removed + [i for i, o in zip(ids, out) if o]))
    return res
