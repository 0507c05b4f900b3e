"""numpy f64 restatement of the two-view pose refinement (csrc/relpose.hip, ov2_relpose_refine_batch), the checker of the
GPU tests: the spherical Sampson residual of E = [t]x R, its analytic Jacobian, the tangent basis of the unit translation,
the left quaternion update and the Levenberg-Marquardt loop with the trust-region rules of the motion-only BA
(oracle/ov2_oracle_pnp.c).  The sums over the pairs are numpy's, not the kernel's fixed tree: results agree to rounding,
iteration logs agree where the problem is tame (tests/test_relpose_ref_cpu.py checks that for every scene a GPU test uses)."""
import math

import numpy as np

TERM_MAX_ITER, TERM_FTOL, TERM_PTOL, TERM_GTOL, TERM_MIN_RADIUS, TERM_FAILURE, TERM_SKIPPED = range(7)

# ov2_ba_default_options: the ceres::Solver::Options the motion-only BA runs with, but for the function tolerance
# (OV2_RELPOSE_FUNCTION_TOLERANCE: Ceres' default instead of the BA's 1e-3)
FTOL, PTOL, MIN_REL = 1e-6, 1e-8, 1e-3
INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS, MIN_DIAG, MAX_DIAG, MAX_INVALID = 1e4, 1e16, 1e-32, 1e-6, 1e32, 5
MIN_PAIRS = 6


def focal_of(K):
    return (float(K[0]) + float(K[1])) / 2.0


def quat_to_R(q):
    """ov2_se3.h quat_to_R (Eigen's toRotationMatrix), q = (x, y, z, w) taken as unit; row-major (9,)"""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, 1 - (txx + tyy)])


def rot_to_quat(R):
    """ov2_se3.h rot_to_quat (the host mirror's branch order), then normalised"""
    R = [float(v) for v in np.asarray(R, np.float64).ravel()]
    t = R[0] + R[4] + R[8]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, 0.25 * s]
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(1.0 + R[0] - R[4] - R[8]) * 2
        q = [0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s]
    elif R[4] > R[8]:
        s = math.sqrt(1.0 + R[4] - R[0] - R[8]) * 2
        q = [(R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s, (R[2] - R[6]) / s]
    else:
        s = math.sqrt(1.0 + R[8] - R[0] - R[4]) * 2
        q = [(R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s, (R[3] - R[1]) / s]
    q = np.array(q)
    return q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def tangent_basis(t):
    """b1 = normalise(e_k x t), k = index of the smallest |t_k| (lowest index on a tie); b2 = t x b1"""
    a = [abs(float(v)) for v in t]
    k = 0
    if a[1] < a[k]:
        k = 1
    if a[2] < a[k]:
        k = 2
    e = np.zeros(3)
    e[k] = 1.0
    b1 = np.cross(e, t)
    b1 = b1 / math.sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2])
    return b1, np.cross(t, b1)


def plus(x, step):
    """x = [t (3, unit), q (4, unit)], step = (w (3), a, b): q <- exp(w) q renormalised, t <- (t + a b1 + b b2) / |...|"""
    t, b = x[:3], x[3:]
    w = step[:3]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < 1e-20:
        th4 = th2 * th2
        imag = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4
        real = 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th4
    else:
        theta = math.sqrt(th2)
        imag = math.sin(0.5 * theta) / theta
        real = math.cos(0.5 * theta)
    a = [imag * w[0], imag * w[1], imag * w[2], real]
    q = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                  a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                  a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    q = q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    b1, b2 = tangent_basis(t)
    tn = t + step[3] * b1 + step[4] * b2
    tn = tn / math.sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2])
    return np.concatenate([tn, q])


def residuals(x, f1, f2, focal, jac=False):
    """r (n,), valid (n,) and, with jac, J (n, 5) of the pairs at x.  A pair whose denominator is not a finite positive
    number is invalid: r = 0, J = 0."""
    t = x[:3]
    R = quat_to_R(x[3:]).reshape(3, 3)
    f1, f2 = np.asarray(f1, np.float64).reshape(-1, 3), np.asarray(f2, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        g = f2 @ R.T                        # R f2
        m = np.cross(t, g)                  # t x g
        w = np.cross(f1, t)                 # f1 x t
        u = w @ R                           # R^T w
        c = (f1 * m).sum(1)
        e = (u * f2).sum(1)
        D = (m * m).sum(1) - c * c + (u * u).sum(1) - e * e
        valid = np.isfinite(D) & (D > 0)
        s = 1.0 / np.sqrt(np.where(valid, D, 1.0))
        r = np.where(valid, focal * c * s, 0.0)
        if not jac:
            return r, valid
        Aw = np.cross(g, w)                                             # dc / dw
        Dw = 2.0 * (np.cross(g, np.cross(m, t)) - (c + e)[:, None] * Aw)   # dD / dw
        At = np.cross(g, f1)                                            # dc / dt
        Dt = 2.0 * (np.cross(g, m) + np.cross(w, f1) - (c + e)[:, None] * At)
        h = (0.5 * c * s * s * s)[:, None]
        Jw = focal * (s[:, None] * Aw - h * Dw)
        Jt = focal * (s[:, None] * At - h * Dt)
        b1, b2 = tangent_basis(t)
        J = np.concatenate([Jw, (Jt @ b1)[:, None], (Jt @ b2)[:, None]], 1)
        J = np.where(valid[:, None], J, 0.0)
    return r, valid, J


def cost_of(x, f1, f2, focal):
    r, _ = residuals(x, f1, f2, focal)
    return 0.5 * float((r * r).sum())


def _chol_solve(A, b):
    """the kernel's Cholesky: (ok, x); a non-positive pivot makes the step invalid"""
    n = len(b)
    L = A.copy()
    ok = True
    for j in range(n):
        d = L[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0.0:
            ok = False
        d = math.sqrt(d if d > 0.0 else 1.0)
        L[j, j] = d
        for i in range(j + 1, n):
            L[i, j] = (L[i, j] - (L[i, :j] * L[j, :j]).sum()) / d
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - (L[i + 1:, i] * y[i + 1:]).sum()) / L[i, i]
    return ok, y


def refine(bv_kf, bv_cur, K, R0, t0, max_iters, skip=None):
    """one frame of ov2_relpose_refine_batch.  returns dict(status, R (9,), t (3,), iters, term, cost (initial, final),
    log [(cost, accepted, radius)] per LM iteration).  status 0 leaves R, t the arguments."""
    f1, f2 = np.asarray(bv_kf, np.float64).reshape(-1, 3), np.asarray(bv_cur, np.float64).reshape(-1, 3)
    if skip is not None:
        keep = np.asarray(skip).reshape(-1) == 0
        f1, f2 = f1[keep], f2[keep]
    R0, t0 = np.array(R0, np.float64).reshape(9), np.array(t0, np.float64).reshape(3)
    out = dict(status=0, R=R0.copy(), t=t0.copy(), iters=0, term=TERM_SKIPPED, cost=(0.0, 0.0), log=[])
    tn = math.sqrt(float(t0 @ t0)) if np.isfinite(t0).all() else float("nan")
    if len(f1) < MIN_PAIRS or not (np.isfinite(f1).all() and np.isfinite(f2).all() and np.isfinite(R0).all()
                                   and np.isfinite(tn) and tn > 0.0):
        return out
    focal = focal_of(K)
    x = np.concatenate([t0 / tn, rot_to_quat(R0)])

    def evaluate(x):
        r, _, J = residuals(x, f1, f2, focal, jac=True)
        return 0.5 * float((r * r).sum()), J.T @ r, J.T @ J

    x_cost, g, H = evaluate(x)
    cost0 = x_cost
    if not math.isfinite(x_cost):
        return out
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    x_norm, radius, dec = -1.0, INITIAL_RADIUS, 2.0
    reuse, invalid, iteration, accepted, term = False, 0, 0, 0, TERM_MAX_ITER
    diag = np.zeros(5)
    log = []
    while True:
        if iteration >= max_iters:
            term = TERM_MAX_ITER
            break
        if radius <= MIN_RADIUS:
            term = TERM_MIN_RADIUS
            break
        iteration += 1
        Hs, gs = H * scale[:, None] * scale[None, :], g * scale
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(Hs), MIN_DIAG), MAX_DIAG)
        reuse = True
        ok, y = _chol_solve(Hs + np.diag(diag / radius), gs)
        step = -y
        model_change = 0.0
        if ok and np.isfinite(step).all():
            model_change = -(float(step @ gs) + 0.5 * float(step @ Hs @ step))
        else:
            ok = False
        if not ok or not model_change > 0.0:
            invalid += 1
            log.append((x_cost, -1, radius))
            if invalid >= MAX_INVALID:
                term = TERM_FAILURE
                break
            radius /= dec
            dec *= 2.0
            continue
        invalid = 0
        cand = plus(x, step * scale)
        cand_cost = cost_of(cand, f1, f2, focal)
        if math.sqrt(float(((x - cand) ** 2).sum())) <= PTOL * (x_norm + PTOL):
            term = TERM_PTOL
            break
        cost_change = x_cost - cand_cost
        if abs(cost_change) <= FTOL * x_cost:
            term = TERM_FTOL
            break
        rel = cost_change / model_change
        if rel > MIN_REL:
            x = cand
            x_norm = math.sqrt(float((x * x).sum()))
            x_cost, g, H = evaluate(x)
            radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            dec, reuse = 2.0, False
            accepted += 1
            log.append((x_cost, 1, radius))
        else:
            radius /= dec
            dec *= 2.0
            log.append((x_cost, 0, radius))
    out.update(iters=iteration, term=term, cost=(cost0, x_cost), log=log)
    if accepted:
        out.update(status=1, R=quat_to_R(x[3:]), t=x[:3].copy())
    return out


# ---- errors against ground truth --------------------------------------------------------------------------------------
def rot_err_deg(R, Rgt):
    c = (np.trace(np.asarray(R).reshape(3, 3).T @ np.asarray(Rgt).reshape(3, 3)) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def dir_err_deg(t, tgt):
    """angle between the translation directions, sign left out (E is the same for t and -t)"""
    c = abs(float(np.dot(t, tgt))) / (np.linalg.norm(t) * np.linalg.norm(tgt))
    return math.degrees(math.acos(min(1.0, c)))
