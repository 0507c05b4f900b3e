"""synthetic 2D-3D scenes for the P3P stage (ov2_p3p_ransac_batch): a 752 x 480 pinhole camera at a random pose, world
points seen inside a 20 px border at depths of 2-25 m, pixel noise, and outliers displaced by 8-60 px in a random
direction.  Seeded, deterministic."""
import numpy as np

from . import synth_ba

K = np.array([458., 458., 367., 248.])
W, H, BORDER = 752, 480, 20


def _bearing(px):
    f = np.stack([(px[:, 0] - K[2]) / K[0], (px[:, 1] - K[3]) / K[1], np.ones(len(px))], 1)
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def _pose(rng):
    R, _ = synth_ba.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 0.2, 3)]))
    return R, rng.normal(0, 1.0, 3)


def make_scene(n, seed=0, outlier_frac=0.2, noise_px=0.3):
    """returns dict: bv (n,3) bearings of the observed pixels, wpts (n,3), px (n,2) observed pixels, R (3,3) / t (3,) the
    camera-to-world pose [R_wc | t_wc], Twc (7,) [t, qx qy qz qw], K (4,), outlier (n,) bool."""
    rng = np.random.default_rng(seed)
    R, t = _pose(rng)
    px = np.stack([rng.uniform(BORDER, W - BORDER, n), rng.uniform(BORDER, H - BORDER, n)], 1)
    depth = rng.uniform(2., 25., n)
    Xc = _bearing(px)
    Xc = Xc / Xc[:, 2:3] * depth[:, None]
    wpts = Xc @ R.T + t
    obs = px + rng.normal(0, noise_px, (n, 2)) if noise_px > 0 else px.copy()
    out = np.zeros(n, bool)
    nbad = int(round(outlier_frac * n))
    if nbad:
        bad = rng.choice(n, nbad, replace=False)
        out[bad] = True
        ang = rng.uniform(0, 2 * np.pi, nbad)
        obs[bad] += (rng.uniform(8., 60., nbad))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return dict(bv=_bearing(obs).reshape(-1, 3), wpts=wpts.reshape(-1, 3), px=obs, R=R, t=t, Twc=synth_ba.pose7(R, t),
                K=K.copy(), outlier=out)


def random_samples(n, seed=0):
    """n exact 3-point samples of the scene generator: bv (n,3,3), X (n,3,3), R (n,3,3), t (n,3) ground truth"""
    rng = np.random.default_rng(seed)
    bv, X, Rs, ts = np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        R, t = _pose(rng)
        px = np.stack([rng.uniform(BORDER, W - BORDER, 3), rng.uniform(BORDER, H - BORDER, 3)], 1)
        f = _bearing(px)
        Xc = f / f[:, 2:3] * rng.uniform(2., 25., 3)[:, None]
        bv[i], X[i], Rs[i], ts[i] = f, Xc @ R.T + t, R, t
    return bv, X, Rs, ts
