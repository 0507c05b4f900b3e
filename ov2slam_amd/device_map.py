"""ctypes mirror of the device map mirror's raw hooks (ov2_map_*, csrc/map.hip) for maps that live ONLY on the device:
no C++ Frame / MapPoint graph beside them.  Used by bench.py (one map per sequence: set-up -> solve -> update of
Optimizer::localBA without the host in the data path, reference src/optimizer.cpp:43-430, 439-735, 741-882) and by the
tests of the batched set-up / update stages.  Plumbing only."""
import ctypes as C

import numpy as np

from . import ba_types as T
from . import synth_ba
from .ba_types import MAX_LOG, BaIterC, BaOptionsC, BaProblemC, BaResultC, dp, i32p, u8p
from .frontend import _check

LM_ALIVE, LM_3D, LM_OBS, LM_KP3D = 1, 2, 4, 8
OBS_ALIVE, OBS_STEREO = 1, 2


class SetupC(C.Structure):
    """ov2_local_ba_setup"""
    _fields_ = [("aborted", C.c_int32), ("n_pose", C.c_int32), ("n_lm", C.c_int32), ("n_res", C.c_int32), ("n_bad", C.c_int32),
                ("pose_kfid", C.c_void_p), ("pose_const", C.c_void_p), ("pose", C.c_void_p), ("lm_lmid", C.c_void_p),
                ("lm", C.c_void_p), ("lm_anchor_pose", C.c_void_p), ("lm_anchor_uv", C.c_void_p), ("res_type", C.c_void_p),
                ("res_pose", C.c_void_p), ("res_lm", C.c_void_p), ("res_uv", C.c_void_p), ("res_sigma", C.c_void_p),
                ("bad_lmid", C.c_void_p), ("res_outlier", C.c_void_p)]


class TemporalC(C.Structure):
    """ov2_map_temporal"""
    _fields_ = [("n_selected", C.c_int32), ("n_candidates", C.c_int32), ("n_good", C.c_int32), ("n_removed", C.c_int32),
                ("good_lmid", C.c_void_p), ("good_wpt", C.c_void_p), ("good_invdepth", C.c_void_p), ("removed_lmid", C.c_void_p)]


class StereoRigC(C.Structure):
    """ov2_stereo_rig"""
    _fields_ = [("Kl", C.c_double * 4), ("Kr", C.c_double * 4), ("Tlr", C.c_double * 7), ("rectified", C.c_int32)]

    @classmethod
    def of(cls, m):
        """the rig of anything with K4 (left), Kr, Tlr, rectified (a synth_stereo_tri map)"""
        r = cls()
        r.Kl[:], r.Kr[:], r.Tlr[:], r.rectified = list(m["K4"]), list(m["Kr"]), list(m["Tlr"]), int(m["rectified"])
        return r


class StereoTriC(C.Structure):
    """ov2_map_stereo_tri"""
    _fields_ = [("n_selected", C.c_int32), ("n_good", C.c_int32), ("n_demoted", C.c_int32), ("good_lmid", C.c_void_p),
                ("good_wpt", C.c_void_p), ("good_invdepth", C.c_void_p), ("demoted_lmid", C.c_void_p), ("demoted_why", C.c_void_p)]


class FilterC(C.Structure):
    """ov2_map_filter"""
    _fields_ = [("n_candidates", C.c_int32), ("n_removed", C.c_int32), ("n_few3d", C.c_int32), ("n_unset3d", C.c_int32),
                ("removed_kfid", C.c_void_p), ("unset3d_lmid", C.c_void_p)]


class LocalIdsC(C.Structure):
    """ov2_map_local_ids"""
    _fields_ = [(n, C.c_int32) for n in ("n_cov", "oldest_cov", "n_fresh", "n_local", "swapped", "extended")] + [
        (n, C.c_void_p) for n in ("cov_kfid", "cov_score", "lmid", "d_lmid", "d_n_local")]


class PgUpdateC(C.Structure):
    """ov2_map_pg_update"""
    _fields_ = [("n_kf_chain", C.c_int32), ("n_kf_younger", C.c_int32), ("n_lm_moved", C.c_int32), ("T_corr", C.c_double * 7)]


class MergeC(C.Structure):
    """ov2_map_merge"""
    _fields_ = [("n_pairs", C.c_int32), ("n_merged", C.c_int32), ("n_skipped", C.c_int32), ("n_rows_moved", C.c_int32),
                ("n_rows_conflict", C.c_int32)]


class SbaCamC(C.Structure):
    """ov2_map_sba_cam"""
    _fields_ = [("calib_l", C.c_double * 4), ("calib_r", C.c_double * 4), ("T_rl", C.c_double * 7)]

    @classmethod
    def of(cls, prob):
        """the calibrations and the extrinsic of a BaProblem (or anything with calib_l, calib_r, T_rl)"""
        c = cls()
        c.calib_l[:], c.calib_r[:], c.T_rl[:] = list(prob.calib_l), list(prob.calib_r), list(prob.T_rl)
        return c


class SbaC(C.Structure):
    """ov2_map_sba"""
    _fields_ = [("n_listed", C.c_int32), ("n_lm", C.c_int32), ("n_skipped", C.c_int32), ("n_res", C.c_int32),
                ("termination", C.c_int32), ("n_log", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("log", BaIterC * MAX_LOG)]


class MatchLocalC(C.Structure):
    """ov2_map_match_local"""
    _fields_ = [(n, C.c_void_p) for n in ("d_kp_off", "d_cand_off", "d_kp_lmid", "d_cand_lmid", "d_match_cand", "d_match_dist",
                                          "d_prev_lmid", "d_new_lmid", "d_n_pairs")]


# OV2_MERGE_* status bytes (include/ov2slam_hip.h)
MERGE_DONE, MERGE_SKIP_RANGE, MERGE_SKIP_SAME, MERGE_SKIP_PREV_DEAD, MERGE_SKIP_NEW_DEAD, MERGE_SKIP_NEW_NOT3D = range(6)
MERGE_NOT_RUN = 255


class DevPairs:
    """device-resident pair lists as ov2_map_merge_points_batch_dev takes them: pair_off (host, B + 1), d_prev / d_new
    (DeviceArray int32 over pair_off[B] slots), d_n_pairs (DeviceArray int32 (B,) or None = whole segments), d_cur_obs
    (DeviceArray uint8 or None)"""

    def __init__(self, pair_off, d_prev, d_new, d_n_pairs=None, d_cur_obs=None):
        self.pair_off = np.ascontiguousarray(pair_off, np.int32)
        self.d_prev, self.d_new, self.d_n_pairs, self.d_cur_obs = d_prev, d_new, d_n_pairs, d_cur_obs


class LooseBaC(C.Structure):
    """ov2_map_loose_ba"""
    _fields_ = [(n, C.c_int32) for n in ("ran", "n_pose", "n_free_pose", "n_lm", "n_res", "n_bad", "n_flagged_left", "n_flagged_right",
                                         "n_removed_obs", "n_stereo_off", "n_removed_lm", "n_written", "n_propagated", "n_kf_younger",
                                         "termination", "n_outliers_pass1", "n_log", "reserved")] + [
        ("T_corr", C.c_double * 7), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("log", BaIterC * MAX_LOG)]


class UpdateC(C.Structure):
    """ov2_local_ba_update"""
    _fields_ = [("n_removed_lm", C.c_int32), ("n_removed_obs", C.c_int32), ("n_stereo_off", C.c_int32),
                ("removed_lmid", C.c_void_p), ("removed_obs", C.c_void_p), ("stereo_off", C.c_void_p)]


def observations_of(prob):
    """the (keyframe, landmark) observations behind a flat BaProblem, as Optimizer::localBA read them off the map:
    returns kf, lm (int32), unpx (n x 2), stereo (uint8), runpx (n x 2), sorted by (kf, lm)"""
    rt, rp, rl = np.asarray(prob.res_type), np.asarray(prob.res_pose, np.int64), np.asarray(prob.res_lm, np.int64)
    uv = np.asarray(prob.res_uv, np.float64).reshape(-1, 2)
    nl = len(prob.lm)
    left = (rt == T.L_XYZ) | (rt == T.L_INV)
    k_of = rp.copy()
    if prob.inv_depth:
        ranch = rt == T.RANCH_INV
        k_of[ranch] = np.asarray(prob.lm_anchor_pose, np.int64)[rl[ranch]]
    nk = len(prob.pose)
    key = k_of * nl + rl
    # left observations: the left blocks + (inverse depth) the anchor observation of every landmark
    lk, luv = key[left], uv[left]
    if prob.inv_depth:
        ak = np.asarray(prob.lm_anchor_pose, np.int64) * nl + np.arange(nl)
        lk = np.concatenate([lk, ak]); luv = np.concatenate([luv, np.asarray(prob.lm_anchor_uv, np.float64).reshape(-1, 2)])
    order = np.argsort(lk, kind="stable")
    lk, luv = lk[order], luv[order]
    assert len(np.unique(lk)) == len(lk) and nk * nl < 2 ** 62
    rk, ruv = key[~left], uv[~left]
    pos = np.searchsorted(lk, rk)
    assert np.all(lk[pos] == rk), "a right-camera block without its left observation"
    stereo = np.zeros(len(lk), np.uint8); stereo[pos] = 1
    run = np.zeros((len(lk), 2)); run[pos] = ruv
    return (lk // nl).astype(np.int32), (lk % nl).astype(np.int32), luv, stereo, run


def world_points_of(prob):
    """initial world points of the landmarks (what MapPoint::ptxyz_ holds before the local BA)"""
    if not prob.inv_depth:
        return np.asarray(prob.lm, np.float64).reshape(-1, 3).copy()
    a = np.asarray(prob.lm_anchor_pose, np.int64)
    z = 1.0 / np.asarray(prob.lm, np.float64).reshape(-1)
    u = np.asarray(prob.lm_anchor_uv, np.float64).reshape(-1, 2)
    K = prob.calib_l
    pc = np.stack([z * (u[:, 0] - K[2]) / K[0], z * (u[:, 1] - K[3]) / K[1], z], 1)
    out = np.zeros((len(z), 3))
    for k in np.unique(a):
        R = synth_ba.quat_to_rot(prob.pose[k, 3:])
        sel = a == k
        out[sel] = pc[sel] @ R.T + prob.pose[k, :3]
    return out


class DeviceMap:
    """one ov2_map filled through the raw hooks"""

    def __init__(self, ctx, max_kf, max_lm, max_obs):
        self.ctx, self.L = ctx, ctx.lib
        h = C.c_void_p()
        _check(ctx.h, self.L.ov2_map_create(ctx.h, int(max_kf), int(max_lm), int(max_obs), C.byref(h)))
        self.h = h
        self.newkf = -1

    @classmethod
    def from_problem(cls, ctx, prob, isobs="newest", spare=(8, 8, 64), scale=None):
        """the map a flat BaProblem was read from: its keyframes, landmarks (at their initial world points) and
        observations.  isobs: 'all' (every MapPoint::isobs_ set, as tests/HostMap builds them), 'newest' (only the landmarks
        the newest keyframe observes: what a live sequence looks like) or 'none'.  spare: capacity beyond the problem
        (keyframes, landmarks, observation rows) before the tables have to grow.  scale: the pyramid level of every observation
        (Keypoint::scale_), in the order of observations_of -- which is the order of the rows; kept as m.row_scale."""
        kf, lm, un, st, run = observations_of(prob)
        scale = None if scale is None else np.ascontiguousarray(scale, np.int32)
        assert scale is None or scale.shape == kf.shape
        nk, nl = len(prob.pose), len(prob.lm)
        m = cls(ctx, nk + spare[0], nl + spare[1], len(kf) + spare[2])
        m.prob, m.newkf = prob, nk - 1
        xyz = world_points_of(prob)
        state = np.full(nl, LM_ALIVE | LM_3D | LM_KP3D, np.uint8)
        if isobs == "all":
            state |= LM_OBS
        elif isobs == "newest":
            state[lm[kf == nk - 1]] |= LM_OBS
        m.set_landmarks(np.arange(nl, dtype=np.int32), xyz, state)
        cut = np.searchsorted(kf, np.arange(nk + 1))
        for k in range(nk):
            a, b = cut[k], cut[k + 1]
            m.add_keyframe(k, prob.pose[k], lm[a:b], un[a:b], run[a:b], st[a:b], None if scale is None else scale[a:b])
        m.row_scale = np.zeros(len(kf), np.int32) if scale is None else scale
        return m

    @classmethod
    def from_temporal_map(cls, ctx, m, spare=(8, 8, 64)):
        """a map of synth_temporal.make_map(dangling=False) as MapManager::attachDevice mirrors the host map built from it:
        every observed landmark alive and seen by the current frame, a 3D map point's keypoints counted as 3D (lm_state_of),
        2D points at the origin"""
        assert not len(m["forget_lm"]) and not len(m["forget_kf"]) and not len(m["forget_kp"]), "dangling references have no mirror form"
        dm = cls(ctx, m["n_kf"] + spare[0], m["n_lm"] + spare[1], len(m["obs_kf"]) + spare[2])
        dm.newkf = int(m["newkf"])
        seen = np.unique(m["obs_lm"]).astype(np.int32)
        is3d = m["lm_3d"][seen].astype(bool)
        st = np.where(is3d, LM_ALIVE | LM_OBS | LM_3D | LM_KP3D, LM_ALIVE | LM_OBS).astype(np.uint8)
        dm.set_landmarks(seen, np.where(is3d[:, None], m["lm_xyz"][seen], 0.0), st)
        for k in range(m["n_kf"]):
            sel = m["obs_kf"] == k
            dm.add_keyframe(k, m["poses"][k], m["obs_lm"][sel], m["obs_uv"][sel].astype(np.float64))
        return dm

    @classmethod
    def from_filter_map(cls, ctx, m, spare=(8, 8, 64), capacity=None, late=0.1):
        """a map of synth_filter.make_map as MapManager::attachDevice mirrors the host map built from it (lm_state_of: 2D points
        at the origin).  A fraction `late` of the rows is appended after all keyframes stand, as merges append them, so that
        the rows of a keyframe are not contiguous.  capacity: (max_kf, max_lm, max_obs) to start from instead of a fit"""
        cap = capacity or (m["n_kf"] + spare[0], m["n_lm"] + spare[1], len(m["obs_kf"]) + spare[2])
        dm = cls(ctx, *cap)
        dm.newkf = int(m["newkf"])
        seen = np.unique(m["obs_lm"]).astype(np.int32)
        st = (LM_ALIVE | np.where(m["lm_3d"][seen] != 0, LM_3D, 0) | np.where(m["lm_isobs"][seen] != 0, LM_OBS, 0)
              | np.where(m["lm_kp3d"][seen] != 0, LM_KP3D, 0)).astype(np.uint8)
        hold = (np.arange(len(m["obs_kf"])) * 7919) % 100 < int(100 * late)
        for k in range(m["n_kf"]):   # (a landmark id beyond the capacity grows the tables here, before its state is set)
            sel = (m["obs_kf"] == k) & ~hold
            dm.add_keyframe(k, m["poses"][k], m["obs_lm"][sel], m["obs_uv"][sel].astype(np.float64))
        for k in np.unique(m["obs_kf"][hold]):
            sel = (m["obs_kf"] == k) & hold
            dm.add_keyframe(int(k), m["poses"][k], m["obs_lm"][sel], m["obs_uv"][sel].astype(np.float64))
        dm.set_landmarks(seen, np.where((m["lm_3d"][seen] != 0)[:, None], m["lm_xyz"][seen], 0.0), st)
        return dm

    @classmethod
    def from_scene(cls, ctx, s, spare=(8, 8, 64), capacity=None):
        """the mirror of a synth_revisit.make_local_map_scene dict, with the match columns, through the public hooks: what
        host_map.LoopMap builds from the same dict.  A map point is 3D when its first keyframe saw it with a 3D keypoint, its
        point is the scene's; `forget_lm` landmarks are removed; a descriptor of `desc` sits on the row of the landmark's
        oldest observer, one of `descs` on the row of the keyframe it names -- where that keyframe does not observe the
        landmark there is no row to carry it and it is left out (MapPoint::addDesc is only ever called for an observer).
        capacity: (max_kf, max_lm, max_obs) to start from instead of a fit"""
        rows = scene_rows(s)
        top_lm = max(int(v["lmid"].max()) for v in s["kps"].values() if len(v["lmid"]))
        cap = capacity or (max(s["kfids"]) + 1 + spare[0], top_lm + 1 + spare[1], sum(len(r["lmid"]) for r in rows.values()) + spare[2])
        m = cls(ctx, *cap)
        m.enable_match_columns()
        m.newkf = int(s["pairs"]["revisit"][0])
        for k in s["kfids"]:
            r = rows[k]
            m.add_keyframe_px(k, s["poses"][k], r["lmid"], r["px"].astype(np.float64), r["px"], r["desc"], r["has_desc"])
        lmid, xyz, state = scene_landmarks(s)
        m.set_landmarks(lmid, xyz, state)
        return m

    def enable_match_columns(self):
        _check(self.ctx.h, self.L.ov2_map_enable_match_columns(self.h))

    def add_keyframe_px(self, kfid, Twc, lmid, unpx, px, desc=None, has_desc=None, runpx=None, is_stereo=None, scale=None):
        """ov2_map_add_keyframe_px: add_keyframe plus the raw pixels (n x 2 float) and, optionally, desc (n x 32) / has_desc (n)"""
        c = np.ascontiguousarray
        Twc, lmid, unpx, px = c(Twc, np.float64), c(lmid, np.int32), c(unpx, np.float64), c(px, np.float32)
        desc = None if desc is None else c(desc, np.uint8).reshape(-1, 32)
        has_desc = None if has_desc is None else c(has_desc, np.uint8)
        assert len(px) == len(lmid) and (desc is None) == (has_desc is None) and (desc is None or len(desc) == len(has_desc) == len(lmid))
        runpx = None if runpx is None else c(runpx, np.float64)
        is_stereo = None if is_stereo is None else c(is_stereo, np.uint8)
        scale = None if scale is None else c(scale, np.int32)
        _check(self.ctx.h, self.L.ov2_map_add_keyframe_px(self.h, int(kfid), self._p(Twc), len(lmid), self._p(lmid), self._p(unpx),
                                                          self._p(runpx), self._p(is_stereo), self._p(scale), self._p(px),
                                                          self._p(desc), self._p(has_desc)))

    def set_obs_desc(self, kfid, lmid, desc, has_desc=None, px=None):
        """ov2_map_set_obs_desc: MapPoint::addDesc for the live rows (kfid[i], lmid[i]); px: None = keep the pixels"""
        c = np.ascontiguousarray
        k, l, d = c(kfid, np.int32).reshape(-1), c(lmid, np.int32).reshape(-1), c(desc, np.uint8).reshape(-1, 32)
        h = np.ones(len(k), np.uint8) if has_desc is None else c(has_desc, np.uint8).reshape(-1)
        px = None if px is None else c(px, np.float32).reshape(-1, 2)
        assert len(k) == len(l) == len(d) == len(h) and (px is None or len(px) == len(k))
        _check(self.ctx.h, self.L.ov2_map_set_obs_desc(self.h, len(k), self._p(k), self._p(l), self._p(px), self._p(d), self._p(h)))

    def download_match_columns(self):
        """dict(obs_kf, obs_lm, obs_flag, obs_px, obs_desc, obs_hasdesc): the rows with their match columns (host copies)"""
        d = self.download()
        n = len(d["obs_kf"])
        out = dict(obs_kf=d["obs_kf"], obs_lm=d["obs_lm"], obs_flag=d["obs_flag"], obs_px=np.zeros((n, 2), np.float32),
                   obs_desc=np.zeros((n, 32), np.uint8), obs_hasdesc=np.zeros(n, np.uint8))
        _check(self.ctx.h, self.L.ov2_map_download_match_columns(self.h, self._p(out["obs_px"]), self._p(out["obs_desc"]),
                                                                 self._p(out["obs_hasdesc"])))
        return out

    def remove_keyframe(self, kfid):
        _check(self.ctx.h, self.L.ov2_map_remove_keyframe(self.h, int(kfid)))

    def enable_local_sets(self, pool_hint=0):
        """ov2_map_enable_local_sets: the map keeps a local id set (Frame::set_local_mapids_) per keyframe from here on"""
        _check(self.ctx.h, self.L.ov2_map_enable_local_sets(self.h, int(pool_hint)))

    def set_local_set(self, kfid, lmids):
        """ov2_map_set_local_set: the set of keyframe kfid becomes `lmids` (any order; stored ascending; duplicates refused)"""
        a = np.ascontiguousarray(lmids, np.int32).reshape(-1)
        _check(self.ctx.h, self.L.ov2_map_set_local_set(self.h, int(kfid), len(a), self._p(a)))

    def get_local_set(self, kfid, cap=None):
        """ov2_map_get_local_set: the stored set of keyframe kfid (ascending), read back from the device.  cap: the entries asked
        for (default: all, in two calls); returns the array, or (array of min(cap, n) ids, n) when cap is given"""
        n = C.c_int()
        if cap is None:
            _check(self.ctx.h, self.L.ov2_map_get_local_set(self.h, int(kfid), 0, None, C.byref(n)))
        out = np.zeros(max(n.value if cap is None else int(cap), 1), np.int32)
        want = n.value if cap is None else int(cap)
        _check(self.ctx.h, self.L.ov2_map_get_local_set(self.h, int(kfid), want, self._p(out), C.byref(n)))
        return out[:n.value].copy() if cap is None else (out[:min(want, n.value)].copy(), n.value)

    def local_pool(self):
        """ov2_map_local_pool: dict(used, capacity, live, squeezes) of the id pool"""
        v = [C.c_int() for _ in range(4)]
        _check(self.ctx.h, self.L.ov2_map_local_pool(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("used", "capacity", "live", "squeezes"), [x.value for x in v]))

    def local_ids_batch(self, others=(), newkf=None, extend=True, nmax_local=0):
        """ov2_map_local_ids_batch on this map and `others` in one call; see local_ids_batch"""
        return local_ids_batch(self.ctx, [self] + list(others), newkf, extend, nmax_local)

    def filter_keyframes_batch(self, others=(), newkf=None, nmin_covscore=25, ratio=0.9):
        """ov2_map_filter_keyframes_batch on this map and `others` in one call; see filter_keyframes_batch"""
        return filter_keyframes_batch(self.ctx, [self] + list(others), newkf, nmin_covscore, ratio)

    def pose_graph_update_batch(self, others=(), newkf=None, chain_kfid=(), chain_Twc=(), want_header=True):
        """ov2_map_pose_graph_update_batch on this map and `others` in one call; see pose_graph_update_batch"""
        return pose_graph_update_batch(self.ctx, [self] + list(others), newkf, chain_kfid, chain_Twc, want_header)

    def local_pose_graph_batch(self, others=(), newkf=None, kfloop_id=(), newTwc=(), stereo=True, options=None, d_n_pairs=None,
                               want=True):
        """ov2_map_local_pose_graph_batch on this map and `others` in one call; see local_pose_graph_batch"""
        return local_pose_graph_batch(self.ctx, [self] + list(others), newkf, kfloop_id, newTwc, stereo, options, d_n_pairs, want)

    def merge_points_batch(self, others=(), pairs=(), cur_obs=None, want_header=True):
        """ov2_map_merge_points_batch on this map and `others` in one call; see merge_points_batch"""
        return merge_points_batch(self.ctx, [self] + list(others), pairs, cur_obs, want_header)

    def structure_ba_batch(self, others=(), lmids=(), cam=None, max_iters=10, want_header=True):
        """ov2_map_structure_ba_batch on this map and `others` in one call: lmids[b] the ids of map b, cam one SbaCamC for
        all maps or one per map (default: of each map's problem); see structure_ba_batch"""
        maps = [self] + list(others)
        cams = [SbaCamC.of(m.prob) for m in maps] if cam is None else (list(cam) if isinstance(cam, (list, tuple)) else [cam] * len(maps))
        return structure_ba_batch(self.ctx, maps, lmids, cams, structure_ba_options(self.ctx, max_iters), want_header)

    def loose_ba_batch(self, others=(), inikfid=None, nkfid=None, cam=None, stereo=True, inv_depth=True, options=None, cur_kfid=None,
                       want=True):
        """ov2_map_loose_ba_batch on this map and `others` in one call: cam one SbaCamC for all maps or one per map (default: of
        each map's problem); see loose_ba_batch"""
        maps = [self] + list(others)
        cams = [SbaCamC.of(m.prob) for m in maps] if cam is None else (list(cam) if isinstance(cam, (list, tuple)) else [cam] * len(maps))
        return loose_ba_batch(self.ctx, maps, inikfid, nkfid, cams, stereo, inv_depth, options, cur_kfid, want)

    def close(self):
        if getattr(self, "h", None):
            self.L.ov2_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def add_keyframe(self, kfid, Twc, lmid, unpx, runpx=None, is_stereo=None, scale=None):
        Twc = np.ascontiguousarray(Twc, np.float64)
        lmid = np.ascontiguousarray(lmid, np.int32)
        unpx = np.ascontiguousarray(unpx, np.float64)
        runpx = None if runpx is None else np.ascontiguousarray(runpx, np.float64)
        is_stereo = None if is_stereo is None else np.ascontiguousarray(is_stereo, np.uint8)
        scale = None if scale is None else np.ascontiguousarray(scale, np.int32)
        _check(self.ctx.h, self.L.ov2_map_add_keyframe(self.h, int(kfid), self._p(Twc), len(lmid), self._p(lmid), self._p(unpx),
                                                       self._p(runpx), self._p(is_stereo), self._p(scale)))

    def set_landmarks(self, lmid, xyz, state):
        lmid = np.ascontiguousarray(lmid, np.int32)
        xyz = None if xyz is None else np.ascontiguousarray(xyz, np.float64)
        state = np.ascontiguousarray(state, np.uint8)
        _check(self.ctx.h, self.L.ov2_map_set_landmarks(self.h, len(lmid), self._p(lmid), self._p(xyz), self._p(state)))

    def remove_obs(self, kfid, lmid):
        k, l = np.ascontiguousarray(kfid, np.int32), np.ascontiguousarray(lmid, np.int32)
        _check(self.ctx.h, self.L.ov2_map_remove_obs(self.h, len(k), self._p(k), self._p(l)))

    def remove_landmarks(self, lmid):
        l = np.ascontiguousarray(lmid, np.int32)
        _check(self.ctx.h, self.L.ov2_map_remove_landmarks(self.h, len(l), self._p(l)))

    def set_isobs(self, lmid, isobs):
        """MapPoint::isobs_ of live landmarks, the other state bits kept"""
        l = np.ascontiguousarray(lmid, np.int32)
        st = self.download()["lm_state"][l]
        st = (st | LM_OBS) if isobs else (st & ~np.uint8(LM_OBS))
        self.set_landmarks(l, None, st.astype(np.uint8))

    def compact(self):
        """ov2_map_compact: (rows before, rows after)"""
        a, b = C.c_int(), C.c_int()
        _check(self.ctx.h, self.L.ov2_map_compact(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def rows(self):
        """ov2_map_obs_rows: (rows, capacity, compactions)"""
        r, c, n = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.h, self.L.ov2_map_obs_rows(self.h, C.byref(r), C.byref(c), C.byref(n)))
        return r.value, c.value, n.value

    def save_state(self):
        _check(self.ctx.h, self.L.ov2_map_save_state(self.h))

    def triangulate_temporal_batch(self, others=(), newkf=None, calib_l=None, stereo=True, max_reproj_err=3.0, want_lists=True):
        """ov2_map_triangulate_temporal_batch on this map and `others` in one call; see triangulate_temporal_batch"""
        return triangulate_temporal_batch(self.ctx, [self] + list(others), newkf, calib_l, stereo, max_reproj_err, want_lists)

    @classmethod
    def from_stereo_tri_map(cls, ctx, m, spare=(8, 8, 64), with_stereo=True):
        """the mirror of a synth_stereo_tri.make_map dict through the public hooks, rows in the dict's order: dead rows and dead
        landmarks included (added alive, then removed).  with_stereo=False: no row carries a stereo flag or a right pixel"""
        dm = cls(ctx, m["n_kf"] + spare[0], m["n_lm"] + spare[1], len(m["obs_kf"]) + spare[2])
        dm.newkf = int(m["newkf"])
        seen = np.unique(m["obs_lm"]).astype(np.int32)
        is3d = m["lm_3d"][seen].astype(bool)
        st = np.where(is3d, LM_ALIVE | LM_OBS | LM_3D | LM_KP3D, LM_ALIVE | LM_OBS).astype(np.uint8)
        dm.set_landmarks(seen, np.where(is3d[:, None], m["lm_xyz"][seen], 0.0), st)
        for k in range(m["n_kf"]):
            sel = m["obs_kf"] == k
            on = m["obs_stereo"][sel] if with_stereo else np.zeros(int(sel.sum()), np.uint8)
            run = np.where(on[:, None] != 0, m["obs_rpx"][sel].astype(np.float64), 0.0)
            dm.add_keyframe(k, m["poses"][k], m["obs_lm"][sel], m["obs_uv"][sel].astype(np.float64), run, on)
        dead = m["obs_alive"] == 0
        if dead.any():
            dm.remove_obs(m["obs_kf"][dead], m["obs_lm"][dead])
        gone = (m["lm_alive"][seen] == 0) | ~np.isin(seen, m["obs_lm"][~dead])   # (a landmark whose every row died goes with them)
        if gone.any():
            dm.remove_landmarks(seen[gone])
        return dm

    def set_obs_stereo(self, kfid, lmid, is_stereo, runpx):
        """ov2_map_set_obs_stereo: flag and undistorted right pixel (float64) of the live rows (kfid[i], lmid[i])"""
        c = np.ascontiguousarray
        k, l, s, r = c(kfid, np.int32), c(lmid, np.int32), c(is_stereo, np.uint8), c(runpx, np.float64)
        _check(self.ctx.h, self.L.ov2_map_set_obs_stereo(self.h, len(k), self._p(k), self._p(l), self._p(s), self._p(r)))

    def triangulate_stereo_batch(self, others=(), newkf=None, rigs=None, max_reproj_err=3.0, want_lists=True):
        """ov2_map_triangulate_stereo_batch on this map and `others` in one call; see triangulate_stereo_batch"""
        return triangulate_stereo_batch(self.ctx, [self] + list(others), newkf, rigs, max_reproj_err, want_lists)

    def download(self):
        """dict of the tables (host copies)"""
        nk, nl, no = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.h, self.L.ov2_map_download(self.h, C.byref(nk), C.byref(nl), C.byref(no), *([None] * 9)))
        K, L, N = nk.value, nl.value, no.value
        d = dict(kf_pose=np.zeros((K, 7)), kf_state=np.zeros(K, np.uint8), lm_xyz=np.zeros((L, 3)), lm_state=np.zeros(L, np.uint8),
                 obs_kf=np.zeros(N, np.int32), obs_lm=np.zeros(N, np.int32), obs_flag=np.zeros(N, np.uint8), obs_uv=np.zeros((N, 2)),
                 obs_ruv=np.zeros((N, 2)))
        _check(self.ctx.h, self.L.ov2_map_download(self.h, None, None, None, *[self._p(d[k]) for k in (
            "kf_pose", "kf_state", "lm_xyz", "lm_state", "obs_kf", "obs_lm", "obs_flag", "obs_uv", "obs_ruv")]))
        return d


def canonical_state(d):
    """a downloaded map (DeviceMap.download) keyed by ids: poses of the live keyframes, (point, state) of the live landmarks,
    the set of live observations with their stereo flag"""
    kfs = {int(k): tuple(d["kf_pose"][k]) for k in np.flatnonzero(d["kf_state"])}
    lms = {int(l): (tuple(d["lm_xyz"][l]), int(d["lm_state"][l])) for l in np.flatnonzero(d["lm_state"] & LM_ALIVE)}
    live = (d["obs_flag"] & OBS_ALIVE).astype(bool)
    if len(live):
        live &= d["kf_state"][d["obs_kf"]].astype(bool) & (d["lm_state"][d["obs_lm"]] & LM_ALIVE).astype(bool)
    obs = {(int(k), int(l)): int(f & OBS_STEREO) for k, l, f in zip(d["obs_kf"][live], d["obs_lm"][live], d["obs_flag"][live])}
    return kfs, lms, obs


def triangulate_temporal_batch(ctx, maps, newkf=None, calib_l=None, stereo=True, max_reproj_err=3.0, want_lists=True):
    """Mapper::triangulateTemporal on the tables of the maps (DeviceMap objects or raw ov2_map handles), keyframe newkf[b]
    (default: each map's newkf) with the left intrinsics calib_l (4,) or (B, 4).  Returns per map dict(selected, candidates,
    good_lmid, good_wpt, good_invdepth, removed_lmid), the lists sorted by lmid -- or None (want_lists=False: asynchronous)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    K = None if calib_l is None else np.ascontiguousarray(np.broadcast_to(np.asarray(calib_l, np.float64), (B, 4)))
    out = (TemporalC * B)() if want_lists else None
    _check(ctx.h, ctx.lib.ov2_map_triangulate_temporal_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p),
                                                             None if K is None else K.ctypes.data_as(C.c_void_p),
                                                             int(bool(stereo)), float(max_reproj_err), out))
    if not want_lists:
        return None

    def fetch(ptr, shape, dt):
        a = np.zeros(shape, dt)
        if a.nbytes:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
        return a
    res = []
    for t in out:
        gl, rl = fetch(t.good_lmid, t.n_good, np.int32), fetch(t.removed_lmid, t.n_removed, np.int32)
        gw, gi = fetch(t.good_wpt, (t.n_good, 3), np.float64), fetch(t.good_invdepth, t.n_good, np.float64)
        o = np.argsort(gl)
        res.append(dict(selected=t.n_selected, candidates=t.n_candidates, good_lmid=gl[o], good_wpt=gw[o], good_invdepth=gi[o],
                        removed_lmid=np.sort(rl)))
    return res


def triangulate_stereo_batch(ctx, maps, newkf=None, rigs=None, max_reproj_err=3.0, want_lists=True):
    """Mapper::triangulateStereo on the tables of the maps (DeviceMap objects or raw ov2_map handles), keyframe newkf[b]
    (default: each map's newkf) with the rigs (one StereoRigC for all maps, or one per map).  Returns per map dict(selected,
    good_lmid, good_wpt, good_invdepth, demoted_lmid, demoted_why), the lists sorted by lmid -- or None (want_lists=False:
    asynchronous)"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    rg = None
    if rigs is not None:
        rg = (StereoRigC * max(B, 1))(*(list(rigs) if isinstance(rigs, (list, tuple)) else [rigs] * B))
    out = (StereoTriC * max(B, 1))() if want_lists else None
    _check(ctx.h, ctx.lib.ov2_map_triangulate_stereo_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), rg, float(max_reproj_err), out))
    if not want_lists:
        return None

    def fetch(ptr, shape, dt):
        a = np.zeros(shape, dt)
        if a.nbytes:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
        return a
    res = []
    for t in out[:B]:
        gl, dl = fetch(t.good_lmid, t.n_good, np.int32), fetch(t.demoted_lmid, t.n_demoted, np.int32)
        gw, gi = fetch(t.good_wpt, (t.n_good, 3), np.float64), fetch(t.good_invdepth, t.n_good, np.float64)
        dw = fetch(t.demoted_why, t.n_demoted, np.uint8)
        o, q = np.argsort(gl), np.argsort(dl)
        res.append(dict(selected=t.n_selected, good_lmid=gl[o], good_wpt=gw[o], good_invdepth=gi[o], demoted_lmid=dl[q],
                        demoted_why=dw[q]))
    return res


def set_obs_stereo_batch_dev(ctx, maps, kfid, d_lmid, d_status, d_rxy, n=None, right_cam=None):
    """ov2_map_set_obs_stereo_batch_dev: the stereo matcher's verdicts onto the rows of keyframe kfid[b] of the maps, from
    device arrays (frontend.DeviceArray, or None with n[b] = 0): d_lmid[b] int32 (n,), d_status[b] uint8 (n,), d_rxy[b] float32
    (n, 2) raw right pixels.  n: entries per map (default: the length of d_lmid[b]).  right_cam: None, one ba_types.CamModelC for
    all maps or one per map.  Asynchronous; the arrays must outlive the stream's passage"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    kf = np.ascontiguousarray(kfid, np.int32)
    nn = np.ascontiguousarray([0 if a is None else a.shape[0] for a in d_lmid] if n is None else n, np.int32)
    ptrs = [(C.c_void_p * max(B, 1))(*[None if a is None else a.ptr for a in arr]) for arr in (d_lmid, d_status, d_rxy)]
    cam = None
    if right_cam is not None:
        cams = list(right_cam) if isinstance(right_cam, (list, tuple)) else [right_cam] * B
        cam = (type(cams[0]) * max(B, 1))(*cams)
    _check(ctx.h, ctx.lib.ov2_map_set_obs_stereo_batch_dev(ctx.h, B, hs, kf.ctypes.data_as(C.c_void_p), nn.ctypes.data_as(C.c_void_p),
                                                           ptrs[0], ptrs[1], ptrs[2], cam))


def filter_keyframes_batch(ctx, maps, newkf=None, nmin_covscore=25, ratio=0.9):
    """Estimator::mapFiltering on the tables of the maps (DeviceMap objects or raw ov2_map handles), keyframe newkf[b] (default:
    each map's newkf) as the new keyframe.  Returns per map dict(candidates, few3d, removed: kfids in removal order,
    unset3d: sorted lmids whose OV2_LM_3D the stage cleared)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    out = (FilterC * B)()
    _check(ctx.h, ctx.lib.ov2_map_filter_keyframes_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), int(nmin_covscore), float(ratio), out))
    res = []
    for f in out:
        rm = np.ctypeslib.as_array(C.cast(f.removed_kfid, i32p), (f.n_removed,)).copy() if f.n_removed else np.zeros(0, np.int32)
        un = np.zeros(f.n_unset3d, np.int32)
        if f.n_unset3d:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, un.ctypes.data_as(C.c_void_p), f.unset3d_lmid, un.nbytes))
        res.append(dict(candidates=f.n_candidates, few3d=f.n_few3d, removed=rm.tolist(), unset3d=np.sort(un).tolist()))
    return res


def local_ids_batch(ctx, maps, newkf=None, extend=True, nmax_local=0, raw=False):
    """MapManager::updateFrameCovisibility + the set assembly of Mapper::matchingToLocalMap on the tables of the maps (DeviceMap
    objects or raw ov2_map handles, all with local sets), keyframe newkf[b] (default: each map's newkf) as the new keyframe
    (ov2_map_local_ids_batch).  Returns per map dict(cov_kfid, cov_score, oldest_cov, n_fresh, swapped, extended, lmid: the
    stored set of the keyframe, ascending, d_lmid / d_n_local: the device addresses of the same list and of its count);
    raw=True: the LocalIdsC array itself"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    out = (LocalIdsC * max(B, 1))()
    _check(ctx.h, ctx.lib.ov2_map_local_ids_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), int(bool(extend)), int(nmax_local), out))
    if raw:
        return out

    def pinned(ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, i32p), (n,)).copy() if n else np.zeros(0, np.int32)
    return [dict(cov_kfid=pinned(u.cov_kfid, u.n_cov), cov_score=pinned(u.cov_score, u.n_cov), oldest_cov=u.oldest_cov, n_fresh=u.n_fresh,
                 swapped=u.swapped, extended=u.extended, lmid=pinned(u.lmid, u.n_local), d_lmid=u.d_lmid, d_n_local=u.d_n_local)
            for u in out[:B]]


def match_local_from_mirror(ctx, maps, newkf, nb3dkps, kp_lists, grids, camera, extend=True, nmax_local=0, cam=None, fmaxprojerr=2.0,
                            fdistratio=0.2, pairs=False, dev=False):
    """Mapper::matchingToLocalMap on mirror-only maps from the new keyframes' keypoint ids and grids alone: local_ids_batch
    builds (and stores) every keyframe's local set, match_local_batch takes the returned lists as its cand_lists.  Returns
    (what match_local_batch returns, the local_ids_batch records).  Arrays are passed on, nothing is computed here."""
    ids = local_ids_batch(ctx, maps, newkf, extend, nmax_local)
    res = match_local_batch(ctx, maps, newkf, nb3dkps, kp_lists, grids, [r["lmid"] for r in ids], camera, cam, fmaxprojerr, fdistratio,
                            pairs, dev)
    return res, ids


def pose_graph_update_batch(ctx, maps, newkf=None, chain_kfid=(), chain_Twc=(), want_header=True):
    """the update stage of Optimizer::localPoseGraph on the tables of the maps (DeviceMap objects or raw ov2_map handles):
    chain_kfid[b] / chain_Twc[b] list the free keyframes of map b's graph (ascending, last = newkf[b]; default: each map's
    newkf) with their optimised poses (n x 7); an empty list leaves the map alone.  Returns per map dict(n_kf_chain,
    n_kf_younger, n_lm_moved, T_corr) -- or None (want_header=False: fully asynchronous)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    ids = [np.ascontiguousarray(k, np.int32).reshape(-1) for k in chain_kfid]
    Ts = [np.ascontiguousarray(t, np.float64).reshape(-1, 7) for t in chain_Twc]
    assert len(ids) == len(Ts) == B and all(len(k) == len(t) for k, t in zip(ids, Ts))
    off = np.concatenate([[0], np.cumsum([len(k) for k in ids])]).astype(np.int32)
    kid = np.ascontiguousarray(np.concatenate(ids + [np.zeros(0, np.int32)]), np.int32)
    Twc = np.ascontiguousarray(np.concatenate(Ts + [np.zeros((0, 7))]), np.float64)
    out = (PgUpdateC * B)() if want_header else None
    _check(ctx.h, ctx.lib.ov2_map_pose_graph_update_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                                          kid.ctypes.data_as(C.c_void_p), Twc.ctypes.data_as(C.c_void_p), out))
    if not want_header:
        return None
    return [dict(n_kf_chain=u.n_kf_chain, n_kf_younger=u.n_kf_younger, n_lm_moved=u.n_lm_moved, T_corr=np.array(u.T_corr[:]))
            for u in out]


def pose_graph_update_batch_dev(ctx, maps, newkf, chain_kfid, d_chain_Twc, d_skip=None, want_header=True):
    """ov2_map_pose_graph_update_batch_dev: pose_graph_update_batch with the optimised poses in device memory.  chain_kfid[b]
    lists the free keyframes of map b (host); d_chain_Twc is ONE device array (DeviceArray, torch tensor or address) holding
    their poses map after map, d_skip (device, one byte per map, or None) the maps to leave alone.  Returns the headers as
    pose_graph_update_batch does -- or None (want_header=False: fully asynchronous)"""
    from .pose_graph import _addr
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    ids = [np.ascontiguousarray(k, np.int32).reshape(-1) for k in chain_kfid]
    assert len(ids) == B
    off = np.concatenate([[0], np.cumsum([len(k) for k in ids])]).astype(np.int32)
    kid = np.ascontiguousarray(np.concatenate(ids + [np.zeros(0, np.int32)]), np.int32)
    out = (PgUpdateC * max(B, 1))() if want_header else None
    _check(ctx.h, ctx.lib.ov2_map_pose_graph_update_batch_dev(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                                              kid.ctypes.data_as(C.c_void_p), C.c_void_p(_addr(d_chain_Twc)),
                                                              C.c_void_p(_addr(d_skip)), out))
    if not want_header:
        return None
    return [dict(n_kf_chain=u.n_kf_chain, n_kf_younger=u.n_kf_younger, n_lm_moved=u.n_lm_moved, T_corr=np.array(u.T_corr[:]))
            for u in out[:B]]


LPG_DONE, LPG_DEGENERATE, LPG_NO_CHAIN = 0, 1, 2   # OV2_LPG_* (include/ov2slam_hip.h)


class LocalPgC(C.Structure):
    """ov2_map_local_pg"""
    _fields_ = [("verdict", C.c_int32), ("kfloop_id", C.c_int32), ("n_pose", C.c_int32), ("reserved", C.c_int32),
                ("update", PgUpdateC), ("result", T.PgResultC)]


def _lpg_args(maps, newkf, kfloop_id, newTwc):
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32).reshape(-1)
    lo = np.ascontiguousarray(kfloop_id, np.int32).reshape(-1)
    Tw = None if newTwc is None else np.ascontiguousarray(newTwc, np.float64).reshape(-1, 7)
    assert len(nk) == B and len(lo) == B and (Tw is None or len(Tw) == B)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return B, hs, (nk, lo, Tw), [p(nk), p(lo), p(Tw)]


def local_pose_graph_batch(ctx, maps, newkf, kfloop_id, newTwc, stereo=True, options=None, d_n_pairs=None, want=True):
    """Optimizer::localPoseGraph(keyframe newkf[b], kfloop_id[b], newTwc[b]) on the tables of the maps (DeviceMap objects or raw
    ov2_map handles) in one call (ov2_map_local_pose_graph_batch): assembly, solve, degenerate gate and update on the device.
    options: a BaOptionsC (None: localPoseGraph's); d_n_pairs: device int32 (B,) whose entries the refused maps clear (DeviceArray,
    torch tensor, address or None).  Returns per map dict(verdict, kfloop_id, n_pose, n_kf_chain, n_kf_younger, n_lm_moved,
    T_corr, result: the PgResultC of the solve, raw: the bytes of the record) -- or None (want=False: nothing synchronises)"""
    from .pose_graph import _addr
    B, hs, keep, args = _lpg_args(maps, newkf, kfloop_id, newTwc)
    out = (LocalPgC * max(B, 1))() if want else None
    _check(ctx.h, ctx.lib.ov2_map_local_pose_graph_batch(ctx.h, B, hs, *args, int(bool(stereo)),
                                                         None if options is None else C.addressof(options),
                                                         C.c_void_p(_addr(d_n_pairs)), out))
    if not want:
        return None
    return [dict(verdict=u.verdict, kfloop_id=u.kfloop_id, n_pose=u.n_pose, n_kf_chain=u.update.n_kf_chain,
                 n_kf_younger=u.update.n_kf_younger, n_lm_moved=u.update.n_lm_moved, T_corr=np.array(u.update.T_corr[:]),
                 result=T.PgResultC.from_buffer_copy(u.result), raw=bytes(u)) for u in out[:B]]


def local_pose_graph_assemble(ctx, maps, newkf, kfloop_id, newTwc):
    """the assembly launch of local_pose_graph_batch alone, downloaded (ov2_map_local_pose_graph_assemble; for tests): per map
    None (no chain) or dict(kfids, pose (n x 7), T_ij (n x 7): the n - 1 odometry edges, then the closing edge)"""
    B, hs, (nk, _, _), args = _lpg_args(maps, newkf, kfloop_id, newTwc)
    cap = int(np.maximum(nk, 0).sum()) + B + 1
    off, kid = np.zeros(B + 1, np.int32), np.zeros(cap, np.int32)
    pose, Tij = np.zeros((cap, 7)), np.zeros((cap, 7))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(ctx.h, ctx.lib.ov2_map_local_pose_graph_assemble(ctx.h, B, hs, *args, cap, p(off), p(kid), p(pose), p(Tij)))
    return [None if off[b] == off[b + 1] else dict(kfids=kid[off[b]:off[b + 1]].copy(), pose=pose[off[b]:off[b + 1]].copy(),
                                                   T_ij=Tij[off[b]:off[b + 1]].copy()) for b in range(B)]


def merge_points_batch(ctx, maps, pairs, cur_obs=None, want_header=True, dev=False):
    """MapManager::mergeMapPoints on the tables of the maps (DeviceMap objects or raw ov2_map handles): pairs[b] is map b's
    ordered list of (prevlmid, newlmid), cur_obs[b] (optional) one flag per pair -- the current frame held prevlmid.
    dev=False: ov2_map_merge_points_batch on host arrays.  dev=True: ov2_map_merge_points_batch_dev, either on the same lists
    uploaded here or on a DevPairs (then cur_obs is the DevPairs' own).  Returns (per map dict(n_pairs, n_merged, n_skipped,
    n_rows_moved, n_rows_conflict), per map uint8 array of OV2_MERGE_* statuses over its segment) -- or None
    (want_header=False: fully asynchronous, nothing is read back)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[getattr(m, "h", m) for m in maps])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if isinstance(pairs, DevPairs):
        assert dev
        dp_ = pairs
    else:
        ps = [np.ascontiguousarray(q, np.int32).reshape(-1, 2) for q in pairs]
        assert len(ps) == B
        off = np.concatenate([[0], np.cumsum([len(q) for q in ps])]).astype(np.int32)
        prev = np.ascontiguousarray(np.concatenate([q[:, 0] for q in ps] + [np.zeros(0, np.int32)]), np.int32)
        new = np.ascontiguousarray(np.concatenate([q[:, 1] for q in ps] + [np.zeros(0, np.int32)]), np.int32)
        cur = None
        if cur_obs is not None:
            cs = [np.zeros(len(q), np.uint8) if c is None else np.ascontiguousarray(c, np.uint8).reshape(-1) for q, c in zip(ps, cur_obs)]
            assert all(len(c) == len(q) for c, q in zip(cs, ps))
            cur = np.ascontiguousarray(np.concatenate(cs + [np.zeros(0, np.uint8)]), np.uint8)
        if dev:
            pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
            dp_ = DevPairs(off, ctx.to_device(pad(prev)), ctx.to_device(pad(new)), None, None if cur is None else ctx.to_device(pad(cur)))
    out = (MergeC * B)() if want_header else None
    if dev:
        total = int(dp_.pair_off[-1]) if B else 0
        d_st = ctx.to_device(np.full(max(total, 1), MERGE_NOT_RUN, np.uint8)) if want_header else None
        ptr = lambda a: None if a is None else a.ptr
        _check(ctx.h, ctx.lib.ov2_map_merge_points_batch_dev(ctx.h, B, hs, p(dp_.pair_off), ptr(dp_.d_prev), ptr(dp_.d_new),
                                                            ptr(dp_.d_cur_obs), ptr(dp_.d_n_pairs), out, ptr(d_st)))
        if not want_header:
            return None
        off, st = dp_.pair_off, d_st.get()[:total]
    else:
        st = np.full(max(int(off[-1]), 1), MERGE_NOT_RUN, np.uint8) if want_header else None
        _check(ctx.h, ctx.lib.ov2_map_merge_points_batch(ctx.h, B, hs, p(off), p(prev), p(new), p(cur), out, p(st)))
        if not want_header:
            return None
    hdr = [dict(n_pairs=u.n_pairs, n_merged=u.n_merged, n_skipped=u.n_skipped, n_rows_moved=u.n_rows_moved,
                n_rows_conflict=u.n_rows_conflict) for u in out]
    return hdr, [st[off[b]:off[b + 1]].copy() for b in range(B)]


class DevIds:
    """device-resident id lists as ov2_map_structure_ba_batch_dev takes them: lm_off (host, B + 1), d_lmid (DeviceArray int32
    over lm_off[B] slots), d_n (DeviceArray int32 (B,) or None = whole segments)"""

    def __init__(self, lm_off, d_lmid, d_n=None):
        self.lm_off = np.ascontiguousarray(lm_off, np.int32)
        self.d_lmid, self.d_n = d_lmid, d_n


def structure_ba_options(ctx, max_iters=10):
    """the options Optimizer::structureOnlyBA runs with (src/optimizer.cpp:2733-2751): those of the local BA, 10 iterations"""
    o = BaOptionsC()
    ctx.lib.ov2_ba_default_options(C.byref(o), 5.9915)
    o.max_iters, o.l2_refine = int(max_iters), 0
    return o


def structure_ba_batch(ctx, maps, lmid_lists, cams, options=None, want_header=True, dev=False, d_status=None):
    """Optimizer::structureOnlyBA on the tables of the maps (DeviceMap objects or raw ov2_map handles): lmid_lists[b] the ids of
    map b, cams[b] its SbaCamC, options a BaOptionsC (default: structure_ba_options).
    dev=False: ov2_map_structure_ba_batch on host lists.  dev=True: ov2_map_structure_ba_batch_dev, either on the same lists
    uploaded here or on a DevIds; d_status (DeviceArray uint8 over the segments, or None) passes over the entries whose byte is
    not OV2_MERGE_DONE.  Returns per map dict(n_listed, n_lm, n_skipped, n_res, termination, n_log, initial_cost, final_cost,
    log: list of dicts as BaResult.log, raw: the bytes of the ov2_map_sba record) -- or None (want_header=False: fully
    asynchronous, nothing is read back)"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    o = structure_ba_options(ctx) if options is None else options
    assert len(cams) == B
    cc = (SbaCamC * max(B, 1))(*cams)
    out = (SbaC * max(B, 1))() if want_header else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ptr = lambda a: None if a is None else a.ptr
    if isinstance(lmid_lists, DevIds):
        assert dev
        ids = lmid_lists
    else:
        ls = [np.ascontiguousarray(q, np.int32).reshape(-1) for q in lmid_lists]
        assert len(ls) == B
        off = np.concatenate([[0], np.cumsum([len(q) for q in ls])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(ls + [np.zeros(0, np.int32)]), np.int32)
        if dev:
            ids = DevIds(off, ctx.to_device(flat if len(flat) else np.zeros(1, np.int32)))
    if dev:
        _check(ctx.h, ctx.lib.ov2_map_structure_ba_batch_dev(ctx.h, B, hs, p(ids.lm_off), ptr(ids.d_lmid), ptr(ids.d_n), ptr(d_status),
                                                            cc, C.byref(o), out))
    else:
        assert d_status is None
        _check(ctx.h, ctx.lib.ov2_map_structure_ba_batch(ctx.h, B, hs, p(off), p(flat), cc, C.byref(o), out))
    if not want_header:
        return None
    return [dict(n_listed=u.n_listed, n_lm=u.n_lm, n_skipped=u.n_skipped, n_res=u.n_res, termination=u.termination, n_log=u.n_log,
                 initial_cost=u.initial_cost, final_cost=u.final_cost,
                 log=[dict(cost=i.cost, cost_change=i.cost_change, radius=i.radius, relative_decrease=i.relative_decrease,
                           model_cost_change=i.model_cost_change, valid=bool(i.step_is_valid), ok=bool(i.step_is_successful))
                      for i in u.log[:u.n_log]], raw=bytes(u)) for u in out[:B]]


def scene_rows(s):
    """kfid -> dict(lmid, px (float32), desc (n x 32), has_desc) of a synth_revisit.make_local_map_scene dict: the observation
    rows of every keyframe with the descriptors they carry (see DeviceMap.from_scene)"""
    first = {}
    for k in sorted(s["kfids"]):
        for l in s["kps"][k]["lmid"].tolist():
            first.setdefault(l, k)
    rows = {}
    for k in s["kfids"]:
        v = s["kps"][k]
        n = len(v["lmid"])
        desc, has = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        for i, l in enumerate(v["lmid"].tolist()):
            d = s["desc"].get(l) if first[l] == k else None
            for q, dq in s.get("descs", {}).get(l, []):     # a later addDesc for a keyframe that already has one is ignored
                if q == k and d is None:
                    d = dq
            if d is not None:
                desc[i], has[i] = d, 1
        rows[k] = dict(lmid=np.ascontiguousarray(v["lmid"], np.int32), px=np.ascontiguousarray(v["uv"], np.float32).reshape(-1, 2),
                       desc=desc, has_desc=has)
    return rows


def scene_landmarks(s):
    """(lmid, xyz, state) of the landmarks of a make_local_map_scene dict as host_map.LoopMap creates them: 3D (and its
    keypoints 3D) when the first keyframe that sees it holds a 3D keypoint, at the scene's point; not alive when forgotten"""
    first = {}
    for k in sorted(s["kfids"]):
        v = s["kps"][k]
        for i, l in enumerate(v["lmid"].tolist()):
            first.setdefault(l, (bool(v["kp3d"][i]), v["xyz"][i]))
    gone = set(int(l) for l in s["forget_lm"])
    lmid = np.array(sorted(first), np.int32)
    is3d = np.array([first[int(l)][0] for l in lmid])
    xyz = np.array([first[int(l)][1] if first[int(l)][0] else np.zeros(3) for l in lmid], np.float64).reshape(-1, 3)
    state = np.where(is3d, LM_ALIVE | LM_OBS | LM_3D | LM_KP3D, LM_ALIVE | LM_OBS).astype(np.uint8)
    state[[int(l) in gone for l in lmid]] = 0
    return lmid, xyz, state


def _match_ids(maps, newkf, nb3dkps, kp_lists, grids, cand_lists):
    """the id arrays of the match calls: grids = (grid_ptr over B * ncells + 1 cells, grid_kp) or None"""
    B = len(maps)
    c = np.ascontiguousarray
    cat = lambda ls: c(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in ls] + [np.zeros(0, np.int32)]), np.int32)
    off = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int32)
    a = dict(hs=(C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps]),
             newkf=c([m.newkf for m in maps] if newkf is None else newkf, np.int32), nb3dkps=c(np.broadcast_to(np.asarray(nb3dkps, np.int32), (B,))),
             kp_off=off(kp_lists), kp_lmid=cat(kp_lists), cand_off=off(cand_lists), cand_lmid=cat(cand_lists),
             grid_ptr=None if grids is None else c(grids[0], np.int32), grid_kp=None if grids is None else c(grids[1], np.int32))
    return a


def _match_call_args(ctx, a, camera, cam):
    K, w, h, cell = camera
    K = np.ascontiguousarray(K, np.float64)
    a["K"] = K
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    return [ctx.h, len(a["kp_off"]) - 1, a["hs"], p(a["newkf"]), p(a["nb3dkps"]), p(a["kp_off"]), p(a["kp_lmid"]), p(a["grid_ptr"]),
            p(a["grid_kp"]), p(a["cand_off"]), p(a["cand_lmid"]), p(K), int(w), int(h), int(cell), None if cam is None else C.addressof(cam)]


def match_gather_batch(ctx, maps, newkf, nb3dkps, kp_lists, grids, cand_lists, camera, cam=None):
    """ov2_map_match_gather_batch_dev on the maps (DeviceMap objects or raw ov2_map handles), then every gathered array
    downloaded: a dict keyed like mapper.MatchBatchInput (Twc, nb3dkps, kp_off, cand_off, kf_off, kp_px, kp_desc_ptr, kp_descs,
    kp_kf_ptr, kp_kfids, kp_kf_px, grid_ptr, grid_kp, cand_wpt, cand_desc_ptr, cand_descs, cand_kf_ptr, cand_kfids, kf_Twc) plus
    kp_lmid / cand_lmid, the device copies of the id lists.  camera = (K4, img_w, img_h, cell).  For tests."""
    from .mapper import MatchBatchInputC
    a = _match_ids(maps, newkf, nb3dkps, kp_lists, grids, cand_lists)
    out, dk, dc = MatchBatchInputC(), C.c_void_p(), C.c_void_p()
    _check(ctx.h, ctx.lib.ov2_map_match_gather_batch_dev(*_match_call_args(ctx, a, camera, cam), C.byref(out), C.byref(dk), C.byref(dc)))
    ctx.synchronize()
    B, nkp, nc = out.B, out.n_kp, out.n_cand

    def get(ptr, shape, dt):
        arr = np.zeros(shape, dt)
        addr = ptr if isinstance(ptr, int) or ptr is None else C.cast(ptr, C.c_void_p).value
        if arr.nbytes and addr:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(addr), arr.nbytes))
        return arr
    g = dict(B=B, n_kp=nkp, n_cand=nc)
    if nkp == 0:
        return g
    g["Twc"], g["nb3dkps"] = get(out.Twc, (B, 7), np.float64), get(out.nb3dkps, B, np.int32)
    for k in ("kp_off", "cand_off", "kf_off"):
        g[k] = get(getattr(out, k), B + 1, np.int32)
    g["kp_px"] = get(out.kp_px, (nkp, 2), np.float32)
    g["kp_desc_ptr"], g["kp_kf_ptr"] = get(out.kp_desc_ptr, nkp + 1, np.int32), get(out.kp_kf_ptr, nkp + 1, np.int32)
    g["kp_descs"] = get(out.kp_descs, (int(g["kp_desc_ptr"][-1]), 32), np.uint8)
    g["kp_kfids"] = get(out.kp_kfids, int(g["kp_kf_ptr"][-1]), np.int32)
    g["kp_kf_px"] = get(out.kp_kf_px, (int(g["kp_kf_ptr"][-1]), 2), np.float32)
    g["cand_wpt"] = get(out.cand_wpt, (nc, 3), np.float64)
    g["cand_desc_ptr"], g["cand_kf_ptr"] = get(out.cand_desc_ptr, nc + 1, np.int32), get(out.cand_kf_ptr, nc + 1, np.int32)
    g["cand_descs"] = get(out.cand_descs, (int(g["cand_desc_ptr"][-1]), 32), np.uint8)
    g["cand_kfids"] = get(out.cand_kfids, int(g["cand_kf_ptr"][-1]), np.int32)
    g["kf_Twc"] = get(out.kf_Twc, (int(g["kf_off"][-1]), 7), np.float64)
    if nc:
        ncell = (len(a["grid_ptr"]) - 1)
        g["grid_ptr"] = get(out.grid_ptr, ncell + 1, np.int32)
        g["grid_kp"] = get(out.grid_kp, int(g["grid_ptr"][-1]), np.int32)
    g["kp_lmid"], g["cand_lmid"] = get(dk.value, nkp, np.int32), get(dc.value, nc, np.int32)
    return g


def match_local_batch(ctx, maps, newkf, nb3dkps, kp_lists, grids, cand_lists, camera, cam=None, fmaxprojerr=2.0, fdistratio=0.2,
                      pairs=False, dev=False):
    """Mapper::matchingToLocalMap from the mirrors (ov2_map_match_local_batch): keyframe newkf[b] of maps[b], its keypoints'
    lmids kp_lists[b] in grid order, grids = (grid_ptr, grid_kp) as ov2_match_batch_input takes them, the unfiltered local ids
    cand_lists[b]; camera = (K4, img_w, img_h, cell).
    dev=False: returns per map (match_lmid, match_dist) over its keypoints, the outputs pre-filled with -7 so that untouched
    slots show.  dev=True: ov2_map_match_local_batch_dev, asynchronous; returns (MatchLocalC, DevPairs or None): with pairs the
    DevPairs is what merge_points_batch(..., dev=True) takes."""
    a = _match_ids(maps, newkf, nb3dkps, kp_lists, grids, cand_lists)
    args = _match_call_args(ctx, a, camera, cam)
    n = int(a["kp_off"][-1])
    if dev:
        out = MatchLocalC()
        _check(ctx.h, ctx.lib.ov2_map_match_local_batch_dev(*args, float(fmaxprojerr), float(fdistratio), int(bool(pairs)), C.byref(out)))
        dp_ = None
        if pairs and out.d_prev_lmid:
            dp_ = DevPairs(a["kp_off"], _DevPtr(out.d_prev_lmid), _DevPtr(out.d_new_lmid), _DevPtr(out.d_n_pairs))
        return out, dp_
    ml, md = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.float32)
    _check(ctx.h, ctx.lib.ov2_map_match_local_batch(*args, float(fmaxprojerr), float(fdistratio), ml.ctypes.data_as(C.c_void_p),
                                                    md.ctypes.data_as(C.c_void_p)))
    o = a["kp_off"]
    return [(ml[o[b]:o[b + 1]].copy(), md[o[b]:o[b + 1]].copy()) for b in range(len(o) - 1)]


class _DevPtr:
    """a device address that somebody else owns, where a DeviceArray's .ptr is expected"""

    def __init__(self, ptr):
        self.ptr = ptr


def fetch_dev(ctx, ptr, shape, dtype):
    """host copy of a device array (one synchronising copy)"""
    arr = np.zeros(shape, dtype)
    if arr.nbytes and ptr:
        _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), arr.nbytes))
    return arr


def restore_state_batch(ctx, maps):
    hs = (C.c_void_p * len(maps))(*[m.h for m in maps])
    _check(ctx.h, ctx.lib.ov2_map_restore_state_batch(ctx.h, len(maps), hs))


def setup_batch(ctx, maps, newkf=None, nmin_covscore=25, nmin_cst_kfs=1, inv_depth=True, calib_l=None):
    """ov2_map_local_ba_setup_batch: returns the array of SetupC device views (one synchronisation for all maps)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[m.h for m in maps])
    nk = np.ascontiguousarray([m.newkf for m in maps] if newkf is None else newkf, np.int32)
    K = None if calib_l is None else np.ascontiguousarray(np.broadcast_to(np.asarray(calib_l, np.float64), (B, 4)))
    out = (SetupC * B)()
    _check(ctx.h, ctx.lib.ov2_map_local_ba_setup_batch(ctx.h, B, hs, nk.ctypes.data_as(C.c_void_p), int(nmin_covscore),
                                                       int(nmin_cst_kfs), int(bool(inv_depth)),
                                                       None if K is None else K.ctypes.data_as(C.c_void_p), out))
    return out


def problems_of(views, proto, inv_depth):
    """ov2_ba_problem[B] (+ ov2_ba_result[B] with the outlier flags inside the maps' blocks) over the device views; proto: a
    BaProblem carrying the calibrations / extrinsic shared by the maps"""
    B = len(views)
    pcs, rcs = (BaProblemC * B)(), (BaResultC * B)()
    for b, v in enumerate(views):
        pc = proto.as_c()
        pc.inv_depth = int(bool(inv_depth))
        pc.n_pose, pc.n_lm, pc.n_res = (0, 0, 0) if v.aborted else (v.n_pose, v.n_lm, v.n_res)
        pc.pose, pc.pose_const, pc.lm = C.cast(v.pose, dp), C.cast(v.pose_const, u8p), C.cast(v.lm, dp)
        pc.lm_anchor_pose, pc.lm_anchor_uv = C.cast(v.lm_anchor_pose, i32p), C.cast(v.lm_anchor_uv, dp)
        pc.res_type, pc.res_pose, pc.res_lm = C.cast(v.res_type, u8p), C.cast(v.res_pose, i32p), C.cast(v.res_lm, i32p)
        pc.res_uv, pc.res_sigma = C.cast(v.res_uv, dp), C.cast(v.res_sigma, dp)
        pcs[b] = pc
        rcs[b].outlier = C.cast(v.res_outlier, u8p)
    return pcs, rcs


def update_batch(ctx, maps, views, cur_kfid=None, want_lists=True, outliers=None):
    """ov2_map_local_ba_update_batch with the outlier flags the solve left in the maps' blocks, or -- outliers[b], a host
    array of n_res flags per map (None: the solve's) -- flags uploaded for the call; returns per map
    dict(removed_lmid, removed_obs (n x 2: kfid, lmid), stereo_off (n x 2)) or None (asynchronous)"""
    B = len(maps)
    hs = (C.c_void_p * B)(*[m.h for m in maps])
    ptrs, owned = [], []
    try:
        for b, v in enumerate(views):
            f = None if outliers is None else outliers[b]
            if v.aborted or f is None:
                ptrs.append(None if v.aborted else v.res_outlier)
                continue
            f = np.ascontiguousarray(f, np.uint8)
            assert f.shape == (v.n_res,)
            d = C.c_void_p()
            _check(ctx.h, ctx.lib.ov2_dev_alloc(ctx.h, max(f.nbytes, 1), C.byref(d)))
            owned.append(d)
            if f.nbytes:
                _check(ctx.h, ctx.lib.ov2_memcpy_h2d(ctx.h, d, f.ctypes.data_as(C.c_void_p), f.nbytes))
            ptrs.append(d.value)
        outl = (C.c_void_p * B)(*ptrs)
        ck = None if cur_kfid is None else np.ascontiguousarray(cur_kfid, np.int32)
        out = (UpdateC * B)() if want_lists else None
        _check(ctx.h, ctx.lib.ov2_map_local_ba_update_batch(ctx.h, B, hs, outl, None if ck is None else ck.ctypes.data_as(C.c_void_p), out))
    finally:
        if owned:   # the update may still be reading them
            ctx.lib.ov2_ctx_synchronize(ctx.h)
            for d in owned:
                ctx.lib.ov2_dev_free(ctx.h, d)
    if not want_lists:
        return None
    res = []
    for u in out:
        def fetch(ptr, n, cols):
            a = np.zeros((n, cols) if cols > 1 else (n,), np.int32)
            if n:
                _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
            return a
        res.append(dict(removed_lmid=np.sort(fetch(u.removed_lmid, u.n_removed_lm, 1)),
                        removed_obs=fetch(u.removed_obs, u.n_removed_obs, 2), stereo_off=fetch(u.stereo_off, u.n_stereo_off, 2)))
    return res


def loose_setup_batch(ctx, maps, inikfid, nkfid, nmin_cst_kfs=1, inv_depth=True, calib_l=None):
    """ov2_map_loose_ba_setup_batch over the keyframes [inikfid[b], nkfid[b]]: returns the array of SetupC device views (one
    synchronisation for all maps)"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    lo, hi = np.ascontiguousarray(inikfid, np.int32).reshape(-1), np.ascontiguousarray(nkfid, np.int32).reshape(-1)
    assert len(lo) == B and len(hi) == B
    K = None if calib_l is None else np.ascontiguousarray(np.broadcast_to(np.asarray(calib_l, np.float64), (B, 4)))
    out = (SetupC * max(B, 1))()
    _check(ctx.h, ctx.lib.ov2_map_loose_ba_setup_batch(ctx.h, B, hs, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                                       int(nmin_cst_kfs), int(bool(inv_depth)),
                                                       None if K is None else K.ctypes.data_as(C.c_void_p), out))
    return out


def loose_ba_options(ctx, robust_mono_th=5.9915, robust=True):
    """ov2_ba_loose_options: the options Optimizer::looseBA runs with (src/optimizer.cpp:1298-1299)"""
    o = BaOptionsC()
    ctx.lib.ov2_ba_loose_options(C.byref(o), float(robust_mono_th), int(bool(robust)))
    return o


def _fetch_lists(ctx, u):
    def fetch(ptr, n, cols):
        a = np.zeros((n, cols) if cols > 1 else (n,), np.int32)
        if n:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
        return a
    return dict(removed_lmid=np.sort(fetch(u.removed_lmid, u.n_removed_lm, 1)), removed_obs=fetch(u.removed_obs, u.n_removed_obs, 2),
                stereo_off=fetch(u.stereo_off, u.n_stereo_off, 2))


_LOOSE_COUNTS = ("ran", "n_pose", "n_free_pose", "n_lm", "n_res", "n_bad", "n_flagged_left", "n_flagged_right", "n_removed_obs",
                 "n_stereo_off", "n_removed_lm", "n_written", "n_propagated", "n_kf_younger", "termination", "n_outliers_pass1", "n_log")


def _loose_records(ctx, out, lists, fetch_lists=True):
    res = []
    for b, u in enumerate(out):
        d = {k: getattr(u, k) for k in _LOOSE_COUNTS}
        d.update(T_corr=np.array(u.T_corr[:]), initial_cost=u.initial_cost, final_cost=u.final_cost,
                 log=[dict(cost=i.cost, cost_change=i.cost_change, radius=i.radius, relative_decrease=i.relative_decrease,
                           model_cost_change=i.model_cost_change, valid=bool(i.step_is_valid), ok=bool(i.step_is_successful))
                      for i in u.log[:u.n_log]], raw=bytes(u))
        if fetch_lists:   # three synchronising copies per map
            d.update(_fetch_lists(ctx, lists[b]))
        res.append(d)
    return res


def loose_update_batch(ctx, maps, views, cur_kfid=None, want=True, outliers=None, fetch_lists=True):
    """ov2_map_loose_ba_update_batch with the outlier flags the solve left in the maps' blocks, or -- outliers[b], a host array
    of n_res flags per map (None: the solve's) -- flags uploaded for the call; returns per map the ov2_map_loose_ba record as
    a dict plus (fetch_lists) removed_lmid, removed_obs (n x 2: kfid, lmid), stereo_off (n x 2) -- or None (want=False:
    asynchronous)"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    ptrs, owned = [], []
    try:
        for b, v in enumerate(views):
            f = None if outliers is None else outliers[b]
            if f is None or v.n_res == 0:
                ptrs.append(v.res_outlier if v.n_res else None)
                continue
            f = np.ascontiguousarray(f, np.uint8)
            assert f.shape == (v.n_res,)
            d = C.c_void_p()
            _check(ctx.h, ctx.lib.ov2_dev_alloc(ctx.h, max(f.nbytes, 1), C.byref(d)))
            owned.append(d)
            _check(ctx.h, ctx.lib.ov2_memcpy_h2d(ctx.h, d, f.ctypes.data_as(C.c_void_p), f.nbytes))
            ptrs.append(d.value)
        outl = (C.c_void_p * max(B, 1))(*ptrs)
        ck = None if cur_kfid is None else np.ascontiguousarray(cur_kfid, np.int32)
        out = (LooseBaC * max(B, 1))() if want else None
        lists = (UpdateC * max(B, 1))() if want else None
        _check(ctx.h, ctx.lib.ov2_map_loose_ba_update_batch(ctx.h, B, hs, outl, None if ck is None else ck.ctypes.data_as(C.c_void_p),
                                                            lists, out))
    finally:
        if owned:   # the update may still be reading them
            ctx.lib.ov2_ctx_synchronize(ctx.h)
            for d in owned:
                ctx.lib.ov2_dev_free(ctx.h, d)
    return _loose_records(ctx, out[:B], lists, fetch_lists) if want else None


def loose_ba_batch(ctx, maps, inikfid, nkfid, cams, stereo=True, inv_depth=True, options=None, cur_kfid=None, want=True, fetch_lists=True):
    """Optimizer::looseBA(inikfid[b], nkfid[b], .) on the tables of the maps (DeviceMap objects or raw ov2_map handles): set-up,
    ov2_ba_solve_batch_dev, update in one call (ov2_map_loose_ba_batch); cams[b] an SbaCamC, options a BaOptionsC (default:
    loose_ba_options).  Returns per map the record dict of loose_update_batch with the solve's termination, costs,
    n_outliers_pass1 and log filled in -- or None (want=False)"""
    B = len(maps)
    hs = (C.c_void_p * max(B, 1))(*[getattr(m, "h", m) for m in maps])
    lo, hi = np.ascontiguousarray(inikfid, np.int32).reshape(-1), np.ascontiguousarray(nkfid, np.int32).reshape(-1)
    assert len(lo) == B and len(hi) == B and len(cams) == B
    o = loose_ba_options(ctx) if options is None else options
    cc = (SbaCamC * max(B, 1))(*cams)
    ck = None if cur_kfid is None else np.ascontiguousarray(cur_kfid, np.int32)
    out = (LooseBaC * max(B, 1))() if want else None
    lists = (UpdateC * max(B, 1))() if want else None
    _check(ctx.h, ctx.lib.ov2_map_loose_ba_batch(ctx.h, B, hs, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), cc,
                                                 int(bool(stereo)), int(bool(inv_depth)), C.byref(o),
                                                 None if ck is None else ck.ctypes.data_as(C.c_void_p), lists, out))
    return _loose_records(ctx, out[:B], lists, fetch_lists) if want else None


def fetch_view(ctx, v, inv_depth):
    """the flat problem of a device view as host arrays keyed like HostMap.setup_local_ba (reference ids, not indices)"""
    def get(ptr, shape, dt):
        a = np.zeros(shape, dt)
        if a.nbytes:
            _check(ctx.h, ctx.lib.ov2_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes))
        return a
    if v.aborted:
        return dict(aborted=True)
    e = 1 if inv_depth else 3
    P, NL, R, NB = v.n_pose, v.n_lm, v.n_res, v.n_bad
    kfid, lmid = get(v.pose_kfid, P, np.int32), get(v.lm_lmid, NL, np.int32)
    anch = get(v.lm_anchor_pose, NL, np.int32)
    return dict(aborted=False, pose_kfid=kfid, pose_const=get(v.pose_const, P, np.uint8), pose=get(v.pose, (P, 7), np.float64),
                lm_lmid=lmid, lm=get(v.lm, (NL, e), np.float64), lm_anchor_kfid=np.where(anch >= 0, kfid[np.maximum(anch, 0)], -1),
                lm_anchor_uv=get(v.lm_anchor_uv, (NL, 2), np.float64), res_type=get(v.res_type, R, np.uint8),
                res_kfid=kfid[get(v.res_pose, R, np.int32)], res_lmid=lmid[get(v.res_lm, R, np.int32)],
                res_uv=get(v.res_uv, (R, 2), np.float64), res_sigma=get(v.res_sigma, R, np.float64),
                bad_lmid=np.sort(get(v.bad_lmid, NB, np.int32)), outlier=get(v.res_outlier, R, np.uint8))
