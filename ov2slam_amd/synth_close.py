"""Seeded scenes for what follows an accepted loop (LoopCloser::closeLoop, reference src/loop_closer.cpp:302-372), built on
synth_revisit.make_local_map_scene(seed): the candidate keyframe 30 with its covisible keyframes, the new keyframe 60 and the
pair list that reaches the 2D-3D half.  The dict is copied, synth_revisit is not touched.  numpy only.

Added to the scene:
  * a covisibility entry for keyframe 10 (the smallest key of keyframe 30's covisibility map, so `inikfid`): (10, 14), which
    makes 14 the keyframe looseBA starts from;
  * pixels that agree with their observers.  The scene's world points are consistent with the new keyframe's true pose only
    (its other pixels are arbitrary: the matcher and the P3P never read them), which leaves structureOnlyBA and looseBA
    without a minimum to find.  Here every keypoint of an older keyframe is the projection of its world point in that
    keyframe's pose, every keypoint of the new keyframe whose landmark an older keyframe sees too is the projection in the
    new keyframe's TRUE pose (`Twc`), and a landmark only the new keyframe sees lies on the ray of its pixel.  The pixels
    of the pairs that the loop is found from are the scene's own.
  * variants of the new keyframe's STORED pose:
      big     the scene's own drift, 0.3 m / 2 degrees: lc_pose_err >= 0.02, looseBA runs
      small   4 mm / 0.06 degrees off the true pose: lc_pose_err < 0.02, no looseBA
  * far_pose(s): a loop pose 6 m from the true one, which the pose graph's degenerate test must refuse."""
import copy

import numpy as np

from . import synth_ba, synth_revisit

LC, NEWKF, INIKF, LOOSE_START = synth_revisit.LC, synth_revisit.NEWKF, 10, 14


def _project(K, R, t, X):
    pc = R.T @ (np.asarray(X, np.float64) - t)
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]]), pc[2]


def make_scene(seed=1, variant="big"):
    assert variant in ("big", "small")
    s = copy.deepcopy(synth_revisit.make_local_map_scene(seed))
    K = np.asarray(s["K4"], np.float64)
    s["cov"] = list(s["cov"]) + [(INIKF, LOOSE_START, 6)]
    Rn, tn = synth_ba.quat_to_rot(np.asarray(s["Twc"][3:])), np.asarray(s["Twc"][:3], np.float64)
    older = set(int(l) for k in s["kfids"] if k != NEWKF for l in s["kps"][k]["lmid"])
    keep = set(q for q, l in s["true_pairs"]) | set(q for q, l in s["vkplmids"])      # the loop is found from these pixels
    for k in s["kfids"]:
        v = s["kps"][k]
        uv, xyz = np.array(v["uv"], np.float64), np.array(v["xyz"], np.float64)
        if k != NEWKF:
            Rk, tk = synth_ba.quat_to_rot(s["poses"][k][3:]), np.asarray(s["poses"][k][:3], np.float64)
            for i, l in enumerate(v["lmid"]):
                p, z = _project(K, Rk, tk, xyz[i])
                assert z > 0.5, (k, int(l), z)
                uv[i] = p
        else:
            for i, l in enumerate(v["lmid"]):
                if int(l) in older:                       # an identity landmark: seen from the true pose
                    p, z = _project(K, Rn, tn, xyz[i])
                    assert z > 0.5
                    if int(l) not in keep:
                        uv[i] = p
                else:                                     # the new keyframe's own landmark: on the ray of its pixel
                    z = 3.0 + 9.0 * ((int(l) * 2654435761) % 1000) / 1000.0
                    xyz[i] = Rn @ np.array([(uv[i, 0] - K[2]) / K[0] * z, (uv[i, 1] - K[3]) / K[1] * z, z]) + tn
                    s["wpt"][int(l)] = xyz[i]
        v["uv"], v["xyz"] = uv.astype(np.float32), xyz
    if variant == "small":
        dR, dt = synth_ba.se3_exp(np.array([0.003, -0.002, 0.002, 0.0006, -0.0007, 0.0004]))
        s["poses"][NEWKF] = synth_ba.pose7(Rn @ dR, tn + dt)
    s["variant"] = variant
    return s


def far_pose(s):
    """a loop pose 6 m from the scene's true one"""
    T = np.array(s["Twc"], np.float64)
    T[:3] += [6.0, 0.0, 0.0]
    return T
