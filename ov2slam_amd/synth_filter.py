"""Seeded maps for the keyframe-culling tests (Estimator::mapFiltering, reference src/estimator.cpp:101-183): nk >= 21
keyframes, the newest one the new keyframe, and a landmark table laid out so that ONE map takes every branch of the stage
with nmin_covscore = 25 at the ratios 0.9 and 0.95.  numpy only.  The stage is index work: pixels and poses are arbitrary.

Keyframes, with N = nk - 1 the new keyframe (the walk goes N-1, N-2, ... down):
  0        redundant (all of its 19 3D landmarks have 5 observers) and covisible with N, but never a candidate
  1 .. 4   older keyframes that share nothing with N: never examined, although they too are redundant
  5 .. N-8 filler keyframes with random landmarks (3D / 2D / is3d_ cleared, seen by N or not, observed or not)
  N-7 'e2' 19 good of 20: kept at 0.95f (equality), removed at 0.9f
  N-6 'e1' 9 good of 10, and two bad landmarks beside them: kept at both ratios (equality at 0.9f)
  N-5 'z'  twelve 3D keypoints, every one a bad landmark (1 observer, 3D, not observed): nbtot == 0, NaN, kept
  N-4 'g'  10 good + 2 landmarks it shares with 'f' alone: 10 of 12 while 'f' stands; once 'f' is gone the two are bad,
           is3d_ is cleared, and 10 of 10 removes 'g'  -> its fate depends on an earlier removal
  N-3 'd'  12 landmarks with exactly 5 observers, 'a' among them: 12 of 12 while 'a' stands, 0 of 12 after -> kept, for
           the same reason
  N-2 'f'  7 3D keypoints < nmin_covscore / 2: removed at once
  N-1 'a'  31 good of 31: removed by the ratio
Covisibility with N comes from one 2D landmark that N and every candidate see (2D keypoints are not counted), and from the
landmarks 'e1' / 'e2' share with N.  The pool of 19 good landmarks is seen by 0 .. 4, which are never removed, so its counts
stay above 4 whatever else goes.
"""
import numpy as np

from . import synth_scene

K4 = synth_scene.K4.copy()
W, H = 752, 480
N_SPECIAL_LM = 50


def make_map(nk=21, nl=60, seed=0):
    """returns a dict:
      n_kf, n_lm, newkf, K4, w, h, poses (nk, 7: t, qx qy qz qw)
      obs_kf, obs_lm (int32), obs_uv (n, 2 float32), sorted by (kf, lm)
      lm_3d, lm_kp3d, lm_isobs (nl uint8): MapPoint::is3d_, Keypoint::is3d_ of its keypoints, MapPoint::isobs_
      lm_xyz (nl, 3)
      roles: dict name -> kfid ('a', 'f', 'd', 'g', 'z', 'e1', 'e2', 'unseen': [1..4]), lm_bad: the landmarks that are bad
      from the start, lm_dep: the two that turn bad once 'f' is gone"""
    assert nk >= 21 and nl >= N_SPECIAL_LM
    rng = np.random.default_rng(seed)
    N = nk - 1
    a, f, d, g, z, e1, e2 = N - 1, N - 2, N - 3, N - 4, N - 5, N - 6, N - 7
    old = [0, 1, 2, 3, 4]
    fillers = list(range(5, N - 7))
    ids = rng.permutation(nl)                    # landmark ids carry no meaning
    take = iter(ids)
    nxt = lambda n: [int(next(take)) for _ in range(n)]
    P, link, w2, w1, b, zz, dd, gg = nxt(19), nxt(1)[0], nxt(1)[0], nxt(1)[0], nxt(2), nxt(12), nxt(12), nxt(2)
    rest = [int(x) for x in take]

    lm_3d, lm_kp3d, lm_isobs = np.ones(nl, np.uint8), np.ones(nl, np.uint8), np.zeros(nl, np.uint8)
    observers = {l: set() for l in range(nl)}
    for l in P:
        observers[l] |= set(old)
    lm_3d[link] = lm_kp3d[link] = 0
    lm_isobs[link] = 1
    observers[link] |= {N, 0, a, f, d, g, z, e1, e2} | set(fillers)
    for l in P:                                  # who else sees the pool
        observers[l] |= {a, e2}
    for l in P[:12]:
        observers[l] |= set(k for k in fillers if rng.random() < 0.5)
    for l in P[:10]:
        observers[l].add(g)
    for l in P[:9]:
        observers[l].add(e1)
    for l in P[:5]:
        observers[l].add(f)
    observers[w2] |= {e2, N}; lm_isobs[w2] = 1
    observers[w1] |= {e1, N}; lm_isobs[w1] = 1
    for l in b:
        observers[l].add(e1)
    for l in zz:
        observers[l].add(z)
    for l in dd:
        observers[l] |= {1, 2, 3, a, d}
    for l in gg:
        observers[l] |= {f, g}
    for l in rest:                               # filler landmarks: only filler keyframes and N see them
        n = int(rng.integers(1, min(8, len(fillers)) + 1))
        observers[l] |= set(int(k) for k in rng.choice(fillers, n, replace=False))
        if rng.random() < 0.5:
            observers[l].add(N)
            lm_isobs[l] = 1
        elif rng.random() < 0.3:
            lm_isobs[l] = 1
        u = rng.random()
        if u < 0.12:
            lm_3d[l] = lm_kp3d[l] = 0            # a 2D point
        elif u < 0.18:
            lm_3d[l] = 0                         # is3d_ cleared by an earlier isBad(), its keypoints still 3D

    obs_kf, obs_lm = [], []
    for l in range(nl):
        for k in sorted(observers[l]):
            obs_kf.append(k); obs_lm.append(l)
    obs_kf, obs_lm = np.array(obs_kf, np.int32), np.array(obs_lm, np.int32)
    o = np.lexsort((obs_lm, obs_kf))
    obs_kf, obs_lm = obs_kf[o], obs_lm[o]
    obs_uv = np.stack([rng.uniform(8, W - 8, len(o)), rng.uniform(8, H - 8, len(o))], 1).astype(np.float32)
    poses = np.zeros((nk, 7))
    poses[:, 0] = 0.1 * np.arange(nk)
    poses[:, 1:3] = rng.normal(0, 0.01, (nk, 2))
    poses[:, 6] = 1.0
    X = np.stack([rng.uniform(-2, 2 + 0.1 * nk, nl), rng.uniform(-1.5, 1.5, nl), rng.uniform(2, 9, nl)], 1)
    return dict(n_kf=nk, n_lm=nl, newkf=N, K4=K4.copy(), w=W, h=H, poses=poses, obs_kf=obs_kf, obs_lm=obs_lm, obs_uv=obs_uv,
                lm_3d=lm_3d, lm_kp3d=lm_kp3d, lm_isobs=lm_isobs, lm_xyz=X,
                roles=dict(a=a, f=f, d=d, g=g, z=z, e1=e1, e2=e2, unseen=[1, 2, 3, 4]),
                lm_bad=sorted(b + zz), lm_dep=sorted(gg))
