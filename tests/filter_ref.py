"""Checker for the keyframe culling stage, written from the reference -- Estimator::mapFiltering (src/estimator.cpp:101-183),
MapManager::removeKeyframe (src/map_manager.cpp:885-919), MapPoint::removeKfObs (src/map_point.cpp:106-126, descriptors aside)
and MapPoint::isBad (src/map_point.cpp:215-234) -- over plain dicts and sets, for the single-threaded loop: bnewkfavailable_
false, no loop closer.  numpy is used for the float division alone.

A map is a dict:
  kfs  {kfid: {lmid: Keypoint::is3d_}}                                   Frame::mapkps_ of the keyframes the map holds
  lms  {lmid: dict(observers=set of kfids, is3d, isobs, kfid)}           MapPoint::set_kfids_, is3d_, isobs_, kfid_ (anchor)
  cov  {kfid: {kfid: count}}                                             Frame::map_covkfs_
"""
import copy

import numpy as np


def build(m):
    """the map of a synth_filter.make_map dict (or any dict with its obs_* / lm_* arrays): every map point created by its
    oldest observer, covisibility counted as MapManager::updateFrameCovisibility counts it"""
    kfs = {k: {} for k in range(m["n_kf"])}
    lms = {}
    for k, l in zip(m["obs_kf"].tolist(), m["obs_lm"].tolist()):
        kfs[k][l] = bool(m["lm_kp3d"][l])
        q = lms.setdefault(l, dict(observers=set(), is3d=bool(m["lm_3d"][l]), isobs=bool(m["lm_isobs"][l]), kfid=k))
        q["observers"].add(k)
        q["kfid"] = min(q["kfid"], k)
    return dict(kfs=kfs, lms=lms, cov=covisibility(kfs, lms))


def covisibility(kfs, lms):
    cov = {k: {} for k in kfs}
    for k, kps in kfs.items():
        for l in kps:
            if l not in lms:
                continue
            for o in lms[l]["observers"]:
                if o != k and o in kfs:
                    cov[k][o] = cov[k].get(o, 0) + 1
    return cov


def is_bad(lm):
    """MapPoint::isBad, side effect included"""
    if len(lm["observers"]) < 2:
        if not lm["isobs"] and lm["is3d"]:
            lm["is3d"] = False
            return True
    if len(lm["observers"]) == 0 and not lm["isobs"]:
        lm["is3d"] = False
        return True
    return False


def remove_kf_obs(lm, kfid):
    """MapPoint::removeKfObs without the descriptors"""
    if kfid not in lm["observers"]:
        return
    lm["observers"].discard(kfid)
    if not lm["observers"]:
        return
    if kfid == lm["kfid"]:
        lm["kfid"] = min(lm["observers"])


def remove_keyframe(M, kfid):
    """MapManager::removeKeyframe"""
    if kfid not in M["kfs"]:
        return
    for l in M["kfs"][kfid]:             # every keypoint, 2D ones included
        if l in M["lms"]:
            remove_kf_obs(M["lms"][l], kfid)
    for co in M["cov"][kfid]:
        if co in M["kfs"]:
            M["cov"][co].pop(kfid, None)
    del M["kfs"][kfid]
    del M["cov"][kfid]


def _ratio_exceeds(good, tot, ratio):
    """float ratio = (float)nbgoodobs / nbtot; ratio > fkf_filtering_ratio_ -- in float, 0 / 0 = NaN compares false"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return bool(np.float32(good) / np.float32(tot) > np.float32(ratio))


def map_filtering(M, newkf, nmin_covscore, ratio, frozen=False):
    """Estimator::mapFiltering on M (edited in place) with keyframe newkf as pnewkf_.  Returns dict(ran, candidates, few3d,
    removed: kfids in removal order, unset3d: landmarks whose is3d_ isBad() cleared, in the order met).
    frozen=True is NOT the reference: it decides every candidate from the counts and flags as they are before the first
    removal and removes afterwards.  It exists so that tests can show their inputs tell the two apart."""
    out = dict(ran=0, candidates=0, few3d=0, removed=[], unset3d=[])
    if np.float32(ratio) >= 1.0:
        return out
    if newkf < 20:
        return out
    out["ran"] = 1
    decide_on = copy.deepcopy(M) if frozen else M
    pending = []
    for kfid in sorted(M["cov"][newkf], reverse=True):     # a copy of map_covkfs_, walked from rbegin()
        if kfid == 0:
            break
        if kfid >= newkf:
            continue
        if kfid not in M["kfs"]:
            M["cov"][newkf].pop(kfid, None)
            continue
        out["candidates"] += 1
        V = decide_on
        kps3d = [l for l, is3d in V["kfs"][kfid].items() if is3d]     # Frame::nb3dkps_ / getKeypoints3d
        if len(kps3d) < nmin_covscore // 2:
            out["few3d"] += 1
            out["removed"].append(kfid)
            pending.append(kfid) if frozen else remove_keyframe(M, kfid)
            continue
        good = tot = 0
        for l in sorted(kps3d):
            lm = V["lms"].get(l)
            if lm is None:                                            # removeMapPointObs(lmid, kfid)
                V["kfs"][kfid].pop(l, None)
                continue
            was3d = lm["is3d"]
            if is_bad(lm):
                if was3d and not lm["is3d"]:
                    out["unset3d"].append(l)
                    M["lms"][l]["is3d"] = False
                continue
            if len(lm["observers"]) > 4:
                good += 1
            tot += 1
        if _ratio_exceeds(good, tot, ratio):
            out["removed"].append(kfid)
            pending.append(kfid) if frozen else remove_keyframe(M, kfid)
    for kfid in pending:
        remove_keyframe(M, kfid)
    return out


def snapshot(M):
    """what the tests compare: observations, observer sets, anchors, is3d_ flags, covisibility maps of the survivors"""
    obs = {(k, l) for k, kps in M["kfs"].items() for l in kps if l in M["lms"]}
    observers = {l: frozenset(q["observers"]) for l, q in M["lms"].items()}
    anchors = {l: q["kfid"] for l, q in M["lms"].items()}
    is3d = {l: q["is3d"] for l, q in M["lms"].items()}
    cov = {k: dict(c) for k, c in M["cov"].items()}
    return dict(kfs=sorted(M["kfs"]), obs=obs, observers=observers, anchors=anchors, is3d=is3d, cov=cov)
