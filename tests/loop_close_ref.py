"""numpy restatement of what follows an accepted loop (reference src/loop_closer.cpp:302-372) and of the update stage of
Optimizer::localPoseGraph (src/optimizer.cpp:2476-2577), for the tests of the chain and of the map-mirror update.  Checker
only: 4 x 4 matrices, nothing shared with the code under test.

A map is a dict:
  poses      {kfid: 7-vector Twc (t, qx qy qz qw)}                 the live keyframes
  points     {lmid: 3-vector}                                       the live landmarks (MapManager::map_plms_)
  obs        iterable of (kfid, lmid)                               live observations
  kp3d       set of lmid whose keypoints carry Keypoint::is3d_
"""
import numpy as np

LCL_FEW_PAIRS, LCL_PG_REFUSED, LCL_CLOSED, LCL_CLOSED_LOOSE_BA = 0, 1, 2, 3


def mat(p7):
    x, y, z, w = np.asarray(p7[3:], float) / np.linalg.norm(p7[3:])
    M = np.eye(4)
    M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    M[:3, 3] = p7[:3]
    return M


def pose7(M):
    """4 x 4 -> (t, qx qy qz qw), qw >= 0 up to the branch (compare poses as matrices, or through same_pose)"""
    R, q = M[:3, :3], np.zeros(4)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q[:] = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return np.concatenate([M[:3, 3], q])


def same_pose(a7, b7, tol):
    """two 7-vectors name the same rigid motion to `tol` (q and -q are the same rotation)"""
    return float(np.abs(mat(a7) - mat(b7)).max()) <= tol


def se3_log_norm(M):
    """|log(M)| of Sophus::SE3::log: (V^-1 t, omega)"""
    R, t = M[:3, :3], M[:3, 3]
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = np.arccos(c)
    W = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    om = 0.5 * W if th < 1e-9 else th / (2.0 * np.sin(th)) * W
    O = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if th < 1e-9:
        Vi = np.eye(3) - 0.5 * O + O @ O / 12.0
    else:
        Vi = np.eye(3) - 0.5 * O + (1.0 - th * np.cos(th / 2) / (2.0 * np.sin(th / 2))) / (th * th) * (O @ O)
    return float(np.linalg.norm(np.concatenate([Vi @ t, om])))


def decide(n_pairs, covis_of_lckf, lckfid, Twc_new_stored, Twc_loop, pairs, pg_accepts, covis_of_inikf=None):
    """the decisions of src/loop_closer.cpp:302-372.  covis_of_*: the keys of Frame::getCovisibleKfMap() (a std::map: the
    smallest key is begin()); an empty map stands for the keyframe's own id (the product's departure: the reference
    dereferences end()).  pg_accepts: what Optimizer::localPoseGraph returned.  Returns dict(branch, inikfid, lc_pose_err,
    merged: the new lmids of the pairs that merge, in list order, loose_start: looseBA's first keyframe or None)"""
    out = dict(branch=LCL_FEW_PAIRS, inikfid=-1, lc_pose_err=0.0, merged=[], loose_start=None)
    if n_pairs < 30:
        return out
    out["inikfid"] = min(covis_of_lckf) if len(covis_of_lckf) else lckfid
    out["lc_pose_err"] = se3_log_norm(np.linalg.inv(mat(Twc_new_stored)) @ mat(Twc_loop))
    if not pg_accepts:
        out["branch"] = LCL_PG_REFUSED
        return out
    out["merged"] = [int(new) for prev, new in pairs if prev != new]
    out["branch"] = LCL_CLOSED
    if out["lc_pose_err"] >= 0.02:
        out["branch"] = LCL_CLOSED_LOOSE_BA
        out["loose_start"] = min(covis_of_inikf) if covis_of_inikf is not None and len(covis_of_inikf) else out["inikfid"]
    return out


def anchors(m):
    """{lmid: its oldest live observer} (MapPoint::kfid_)"""
    a = {}
    for k, l in m["obs"]:
        if k in m["poses"] and l in m["points"]:
            a[l] = min(a.get(l, k), k)
    return a


def update(m, newkf, chain):
    """the update stage: chain = {kfid: optimised 7-vector} of the free keyframes (newkf among them).  Returns (poses:
    {kfid: 4 x 4} of every live keyframe, points: {lmid: 3-vector}, moved_chain, moved_younger: sets of lmid, T_corr 4 x 4)"""
    old = {k: mat(p) for k, p in m["poses"].items()}
    ini = np.linalg.inv(old[newkf])
    opt = mat(chain[newkf])
    new = dict(old)
    for k in old:
        if k in chain:
            new[k] = mat(chain[k])
        elif k > newkf:
            new[k] = opt @ (ini @ old[k])
    points = {l: np.asarray(p, float).copy() for l, p in m["points"].items()}
    moved_chain, moved_younger = set(), set()
    for l, a in anchors(m).items():
        if l not in m["kp3d"] or not (a in chain or a > newkf):
            continue
        cam = np.linalg.inv(old[a]) @ np.append(points[l], 1.0)
        points[l] = (new[a] @ cam)[:3]
        (moved_chain if a in chain else moved_younger).add(l)
    return new, points, moved_chain, moved_younger, opt @ ini
