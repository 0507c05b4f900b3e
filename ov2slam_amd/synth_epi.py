"""synthetic two-view scenes for the epipolar filter (ov2_epipolar_filter_batch): the last keyframe at the origin, the
current frame at (R, t) (X_kf = R X_cur + t), points in front of both, pixel noise, and outliers displaced across the
true epipolar line so that their true score is well above the RANSAC threshold.  Seeded, deterministic."""
import numpy as np

from . import synth_ba

K_EUROC = np.array([458.654, 457.296, 367.215, 248.375])


def _bearings(u, K):
    """Keypoint::bv_ = iK * (unpx, 1), normalised, from the float pixels"""
    u32 = np.asarray(u, np.float32)
    f = np.stack([(u32[:, 0] - K[2]) / K[0], (u32[:, 1] - K[3]) / K[1], np.ones(len(u32))], 1)
    return f / np.linalg.norm(f, axis=1, keepdims=True), u32


def _project(K, X):
    return K[:2] * X[:, :2] / X[:, 2:3] + K[2:]


def _views(n, R, t, K, rng, noise_px, outlier_frac):
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2.5, 12, n)], 1)
    Xc = (X - t) @ R                        # R^T (X - t)
    ukf, ucur = _project(K, X), _project(K, Xc)
    nz_kf, nz_cur = rng.normal(0, noise_px, (n, 2)), rng.normal(0, noise_px, (n, 2))
    ukf, ucur = ukf + nz_kf, ucur + nz_cur
    out = np.zeros(n, bool)
    n_bad = int(round(outlier_frac * n))
    bad = rng.choice(n, n_bad, replace=False) if n_bad else np.zeros(0, int)
    out[bad] = True
    if n_bad:
        # epipolar line of the keyframe pixel in the current image: l = F^T (u_kf, 1), F = K^-T [t]x R K^-1
        Ki = np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.]]))
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        F = Ki.T @ tx @ R @ Ki
        l = np.concatenate([ukf[bad], np.ones((n_bad, 1))], 1) @ F
        nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
        ucur[bad] += nrm * (rng.uniform(25, 80, n_bad) * rng.choice([-1., 1.], n_bad))[:, None]
    noise = np.maximum(np.abs(nz_kf).max(1), np.abs(nz_cur).max(1))
    fkf, ukf32 = _bearings(ukf, K)
    fcur, ucur32 = _bearings(ucur, K)
    return fkf, fcur, ukf32, ucur32, out, noise


def make_scene(n, seed=0, rot_deg=5.0, baseline=0.3, noise_px=0.3, outlier_frac=0.2, n_gate=0, gate_outlier_frac=0.2,
               K=K_EUROC):
    """returns dict: bv_kf, bv_cur (n,3), unpx_kf, unpx_cur (n,2 float32), R (3,3), t (3,) unit, K (4,), outlier (n,) bool,
    noise (n,) largest |pixel noise| of the pair, and the 2D-only gate points gate_kf, gate_cur (n_gate,2 float32),
    gate_outlier (n_gate,) bool."""
    rng = np.random.default_rng(seed)
    K = np.asarray(K, np.float64)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), np.deg2rad(rot_deg) * axis]))
    d = rng.normal(size=3)
    d[2] = abs(d[2]) * 0.3
    t = baseline * d / np.linalg.norm(d)
    fkf, fcur, ukf, ucur, out, noise = _views(n, R, t, K, rng, noise_px, outlier_frac)
    gkf = gcur = np.zeros((0, 2), np.float32)
    gout = np.zeros(0, bool)
    if n_gate:
        _, _, gkf, gcur, gout, _ = _views(n_gate, R, t, K, rng, noise_px, gate_outlier_frac)
    tn = np.linalg.norm(t)
    return dict(bv_kf=fkf, bv_cur=fcur, unpx_kf=ukf, unpx_cur=ucur, R=R, t=t / tn if tn > 0 else t, K=K, outlier=out,
                noise=noise, gate_kf=gkf, gate_cur=gcur, gate_outlier=gout)


def essential(R, t):
    """E = [t]x R (bv_kf^T E bv_cur = 0), ||E||_F = 1"""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def random_samples(n, seed=0):
    """n exact 5-point samples of random non-planar two-view scenes: bv1, bv2 (n,5,3), E (n,3,3) ground truth"""
    rng = np.random.default_rng(seed)
    bv1, bv2, Es = np.zeros((n, 5, 3)), np.zeros((n, 5, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        axis = rng.normal(size=3)
        R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), rng.uniform(0.02, 0.5) * axis / np.linalg.norm(axis)]))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-2, 2, 5), rng.uniform(3, 10, 5)], 1)
        Xc = (X - t) @ R
        bv1[i] = X / np.linalg.norm(X, axis=1, keepdims=True)
        bv2[i] = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
        Es[i] = essential(R, t)
    return bv1, bv2, Es
