"""numpy f64 restatement of the per-frame epipolar filter (csrc/epipolar.hip), the checker of the GPU tests.

The rules are those of VisualFrontEnd::epipolar2d2dFiltering (reference src/visual_front_end.cpp:446-655) and OpenGV's
Ransac<CentralRelativePoseSacProblem> with NISTER, restated from OpenGV's published source, with this project's sampler
(include/ov2slam_hip.h, ov2_epipolar_filter_batch).  The 5-point solver here is deliberately another method than the
kernel's Nister reduction: Stewenius' action matrix (grevlex Groebner basis, eigenvectors through np.linalg.eig), and
the essential matrices are decomposed through an SVD as OpenGV does.  The scoring, the sampler, the RANSAC loop and the
Sampson gate use the kernel's operation order, so that integer outcomes agree exactly."""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
EPS = np.finfo(np.float64).eps


# ---- sampler ------------------------------------------------------------------------------------------------------------
def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def epi_hash(seed, d, j, n):
    a = mix64(seed + GOLD * (d + 1))
    x = mix64(a + GOLD * (j + 1))
    return ((x >> 32) * n) >> 32


def draw(seed, d, n):
    """the 5 distinct indices of draw d (redraw on a duplicate; after 256 attempts the smallest unused index)."""
    idx, j = [], 0
    for _ in range(5):
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
    """2 (1 - cos(atan(errth / focal))): focal = (fx + fy) / 2 and the quotient in float (src/multi_view_geometry.cpp:654-658);
    the unqualified atan / cos of that file are the C library's double functions."""
    focal = np.float32(np.float32(fx) + np.float32(fy))
    focal = np.float32(np.float64(focal) / 2.)
    q = np.float32(np.float32(errth) / focal)
    return 2.0 * (1.0 - math.cos(math.atan(float(q))))


# ---- score (triangulate2 + normalised reprojections), the kernel's operation order -----------------------------------
def score(R, t, f1, f2):
    f1 = np.atleast_2d(f1)
    f2 = np.atleast_2d(f2)
    a0, a1, a2 = f1[:, 0], f1[:, 1], f1[:, 2]
    u = [R[3 * i] * f2[:, 0] + R[3 * i + 1] * f2[:, 1] + R[3 * i + 2] * f2[:, 2] for i in range(3)]
    a00 = a0 * a0 + a1 * a1 + a2 * a2
    a10 = a0 * u[0] + a1 * u[1] + a2 * u[2]
    a01 = -a10
    a11 = -(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    b0 = t[0] * a0 + t[1] * a1 + t[2] * a2
    b1 = t[0] * u[0] + t[1] * u[1] + t[2] * u[2]
    with np.errstate(all="ignore"):
        invdet = 1. / (a00 * a11 - a01 * a10)
        l0 = (a11 * invdet) * b0 + (-a01 * invdet) * b1
        l1 = (-a10 * invdet) * b0 + (a00 * invdet) * b1
        X = [(l0 * f1[:, k] + (t[k] + l1 * u[k])) / 2. for k in range(3)]
        ti = [-(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]) for k in range(3)]
        Xb = [R[k] * X[0] + R[3 + k] * X[1] + R[6 + k] * X[2] + ti[k] for k in range(3)]
        n1 = np.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
        n2 = np.sqrt(Xb[0] * Xb[0] + Xb[1] * Xb[1] + Xb[2] * Xb[2])
        e1 = 1.0 - (f1[:, 0] * (X[0] / n1) + f1[:, 1] * (X[1] / n1) + f1[:, 2] * (X[2] / n1))
        e2 = 1.0 - (f2[:, 0] * (Xb[0] / n2) + f2[:, 1] * (Xb[1] / n2) + f2[:, 2] * (Xb[2] / n2))
    return e1 + e2


# ---- Stewenius' 5-point solver -----------------------------------------------------------------------------------------
# grevlex order of the 20 monomials x^a y^b z^c of degree <= 3
GREVLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
           (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(A, B):
    out = np.zeros((4, 4, 4))
    for a, b, c in zip(*np.nonzero(A)):
        out[a:, b:, c:] += A[a, b, c] * B[:4 - a, :4 - b, :4 - c]
    return out


def fivept_stewenius(f1, f2, return_eig=False):
    """essential matrices (||E||_F = 1, f1^T E f2 = 0) of the 5 pairs, real solutions only (and, with return_eig, the
    10 eigenvalues of the action matrix)."""
    Q = np.einsum("ia,ib->iab", f1, f2).reshape(5, 9)
    N = np.linalg.svd(Q)[2][5:]          # X, Y, Z, W
    E = []
    for e in range(9):
        p = np.zeros((4, 4, 4))
        p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = N[0, e], N[1, e], N[2, e], N[3, e]
        E.append(p)
    E = [E[0:3], E[3:6], E[6:9]]
    EE = [[sum(_pmul(E[i][k], E[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EE[0][0] + EE[1][1] + EE[2][2]
    rows = []
    for i in range(3):
        for j in range(3):
            rows.append(sum(_pmul(2. * EE[i][k] - (tr if i == k else 0.), E[k][j]) for k in range(3)))
    det = (_pmul(_pmul(E[1][1], E[2][2]) - _pmul(E[1][2], E[2][1]), E[0][0])
           - _pmul(_pmul(E[1][0], E[2][2]) - _pmul(E[1][2], E[2][0]), E[0][1])
           + _pmul(_pmul(E[1][0], E[2][1]) - _pmul(E[1][1], E[2][0]), E[0][2]))
    rows.append(det)
    M = np.array([[r[m] for m in GREVLEX] for r in rows])
    try:
        Bm = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return ([], np.zeros(0)) if return_eig else []
    # basis x^2 xy xz y^2 yz z^2 x y z 1; multiplication by x
    A = np.zeros((10, 10))
    A[:6] = -Bm[:6]
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1.
    w, V = np.linalg.eig(A)
    out = []
    for k in range(10):
        if w[k].imag != 0. or V[9, k] == 0:
            continue
        v = V[:, k].real
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        Ek = x * N[0] + y * N[1] + z * N[2] + N[3]
        out.append(Ek / np.linalg.norm(Ek))
    return (out, w) if return_eig else out


def model(f1, f2):
    """OpenGV computeModelCoefficients (NISTER) with this project's tie rule: (ok, R (9,), t (3,))."""
    Wm = np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]])
    cands = []
    for E in fivept_stewenius(f1, f2):
        U, s, Vt = np.linalg.svd(E.reshape(3, 3))
        Ra, Rb = U @ Wm @ Vt, U @ Wm.T @ Vt
        if np.linalg.det(Ra) < 0:
            Ra = -Ra
        if np.linalg.det(Rb) < 0:
            Rb = -Rb
        ta = U[:, 2].copy()
        for R, t in ((Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta)):
            R = R.ravel()
            q = 0.
            for k in range(5):
                q += score(R, t, f1[k], f2[k])[0]
            cands.append((q, R, t))
    qs = [c[0] for c in cands if c[0] == c[0]]
    if not qs:
        return False, None, None
    bq = min(qs)
    best, btr = None, -np.inf
    for q, R, t in cands:
        if q <= bq + 1e-9 and R[0] + R[4] + R[8] > btr:
            btr, best = R[0] + R[4] + R[8], (R, t)
    return True, best[0], best[1]


# ---- RANSAC + gate (one frame of ov2_epipolar_filter_batch) ------------------------------------------------------------
def ransac(bv_kf, bv_cur, nmaxiter, th, seed):
    """OpenGV Ransac::computeModel with the project's sampler: (best_R, best_t, info [iterations, skipped, d, count])."""
    n = len(bv_kf)
    it, skipped, k, best, best_d, bm = 0, 0, 1.0, -(2 ** 31 - 1), -1, None
    max_skip = 10 * nmaxiter
    d = 0
    if n >= 8:
        while it < k and skipped < max_skip:
            idx = draw(seed, d, n)
            ok, R, t = model(bv_kf[idx], bv_cur[idx])
            if not ok:
                skipped += 1
                d += 1
                continue
            cnt = int((score(R, t, bv_kf, bv_cur) < th).sum())
            if cnt > best:
                best, best_d, bm = cnt, d, (R, t)
                w = best / n
                p = min(max(EPS, 1.0 - w ** 5.0), 1.0 - EPS)
                k = math.log(1.0 - 0.99) / math.log(p)
            it += 1
            d += 1
            if it > nmaxiter:
                break
    return bm, [it, skipped, best_d, best if best_d >= 0 else 0]


def fundamental(R, t, K):
    fx, fy, cx, cy = K
    ki = [1. / fx, 0., -cx / fx, 0., 1. / fy, -cy / fy, 0., 0., 1.]
    E = [0.] * 9
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            E[3 * i + j] = t[i1] * R[3 * i2 + j] - t[i2] * R[3 * i1 + j]
    T1 = [ki[i] * E[j] + ki[3 + i] * E[3 + j] + ki[6 + i] * E[6 + j] for i in range(3) for j in range(3)]
    return [T1[3 * i] * ki[j] + T1[3 * i + 1] * ki[3 + j] + T1[3 * i + 2] * ki[6 + j] for i in range(3) for j in range(3)]


def sampson(F, cur, kf):
    """computeSampsonDistance(F, cur, kf) with its float roundings (src/multi_view_geometry.cpp:798-813); vectorised."""
    cur = np.asarray(cur, np.float32).reshape(-1, 2).astype(np.float64)
    kf = np.asarray(kf, np.float32).reshape(-1, 2).astype(np.float64)
    l0, l1, r0, r1 = cur[:, 0], cur[:, 1], kf[:, 0], kf[:, 1]
    rF = [r0 * F[j] + r1 * F[3 + j] + 1. * F[6 + j] for j in range(3)]
    Fl = [F[3 * i] * l0 + F[3 * i + 1] * l1 + F[3 * i + 2] * 1. for i in range(3)]
    f32 = np.float32
    num = (rF[0] * l0 + rF[1] * l1 + rF[2] * 1.).astype(f32)
    num = num * num
    x1, x2, y1, y2 = rF[0].astype(f32), Fl[0].astype(f32), rF[1].astype(f32), Fl[1].astype(f32)
    den = x1 * x1 + y1 * y1 + x2 * x2 + y2 * y2
    with np.errstate(all="ignore"):
        return np.sqrt(num / den)


def epipolar_filter(bv_kf, bv_cur, K, nmaxiter, errth, seed, gate_kf=None, gate_cur=None):
    """one frame: dict(status, R, t, outlier, gate_bad, info, th, dist)."""
    bv_kf, bv_cur = np.asarray(bv_kf, np.float64).reshape(-1, 3), np.asarray(bv_cur, np.float64).reshape(-1, 3)
    n = len(bv_kf)
    ng = 0 if gate_kf is None else len(np.asarray(gate_kf).reshape(-1, 2))
    th = threshold(errth, K[0], K[1])
    bm, info = ransac(bv_kf, bv_cur, nmaxiter, th, seed)
    ninl = info[3]
    status = 0 if (bm is None or ninl < 10) else (1 if 2 * (n - ninl) > n else 2)
    out = np.zeros(n, bool)
    gate = np.zeros(ng, bool)
    dist = None
    R = t = None
    if status >= 1:
        R, t = bm
        out = ~(score(R, t, bv_kf, bv_cur) < th)
    if status == 2 and ng:
        F = fundamental(R, t, K)
        dist = sampson(F, gate_cur, gate_kf)
        gate = dist > np.float32(errth)
    return dict(status=status, R=R, t=t, outlier=out, gate_bad=gate, info=info, th=th, dist=dist)


# ---- VisualFrontEnd::epipolar2d2dFiltering, steps 1-11 (src/visual_front_end.cpp:446-655) -----------------------------
def se3_rotation(q):
    """SE3::rotation of the C++ mirror (quaternion x y z w, normalised first)"""
    x, y, z, w = (float(v) for v in q)
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def bearing(px, K):
    """Frame::computeKeypoint without distortion: bv = iK (unpx, 1), normalised"""
    hx, hy = float(np.float32(px[0])), float(np.float32(px[1]))
    b = ((hx - K[2]) / K[0], (hy - K[3]) / K[1], 1.0)
    nrm = math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    return [b[0] / nrm, b[1] / nrm, b[2] / nrm]


def epipolar2d2d(kf, cur, K, Rkfcur, stereo, nmaxiter, errth, seed):
    """the reference function on two frames.  kf / cur: {lmid: (undistorted pixel (2,) float32, is3d)}; Rkfcur = Rcw(kf) Rwc(cur)
    row-major.  Pairs in ascending lmid order.  returns (removed lmids ascending, status: -1 returned before the RANSAC)"""
    f32 = np.float32
    nbkps = len(cur)
    if nbkps < 8:                                                         # :462
        return [], -1
    nb3d = sum(1 for v in cur.values() if v[1])
    epifrom3dkps = stereo and nb3d > 30                                   # :484
    ids, bkf, bcur = [], [], []
    avg, npar = f32(0.), 0
    for lmid in sorted(cur):                                              # :493-519
        px, is3d = cur[lmid]
        if epifrom3dkps and not is3d:
            continue
        if lmid not in kf:                                                # kfkp.lmid_ != kp.lmid_
            continue
        b = bearing(px, K)
        ids.append(lmid)
        bkf.append(bearing(kf[lmid][0], K))
        bcur.append(b)
        r = [Rkfcur[3 * i] * b[0] + Rkfcur[3 * i + 1] * b[1] + Rkfcur[3 * i + 2] * b[2] for i in range(3)]
        invz = 1. / r[2]
        u, v = f32(K[0] * (r[0] * invz) + K[2]), f32(K[1] * (r[1] * invz) + K[3])   # projCamToImage -> cv::Point2f
        dx, dy = f32(u - f32(kf[lmid][0][0])), f32(v - f32(kf[lmid][0][1]))
        avg = f32(float(avg) + math.sqrt(float(dx) * float(dx) + float(dy) * float(dy)))   # float += cv::norm
        npar += 1
    if nbkps < 8:                                                         # :521, the first test again
        return [], -1
    with np.errstate(all="ignore"):
        avg = f32(avg / f32(npar))                                        # :528
    if float(avg) < 2. * float(f32(errth)):                               # :530
        return [], -1
    gids, gkf, gcur = [], [], []
    if epifrom3dkps:                                                      # :611-648: every 2D keypoint, the keyframe's
        for lmid in sorted(cur):                                          # keypoint of the same id or a default one
            px, is3d = cur[lmid]
            if is3d:
                continue
            gids.append(lmid)
            gkf.append(kf[lmid][0] if lmid in kf else np.zeros(2, f32))
            gcur.append(px)
    r = epipolar_filter(np.array(bkf).reshape(-1, 3), np.array(bcur).reshape(-1, 3), K, nmaxiter, errth, seed,
                        np.array(gkf, f32).reshape(-1, 2), np.array(gcur, f32).reshape(-1, 2))
    if r["status"] < 2:                                                   # :573-585
        return [], r["status"]
    removed = [ids[i] for i in np.flatnonzero(r["outlier"])] + [gids[i] for i in np.flatnonzero(r["gate_bad"])]
    return sorted(removed), r["status"]
