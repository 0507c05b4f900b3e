"""ctypes driver of the C++ host mirror (libov2host.so, ov2slam_amd/host/): builds a Frame/MapPoint graph, runs
Optimizer::setupLocalBA on the CPU or Estimator::applyLocalBA on the GPU.  Used by tests and bring-up only."""
import ctypes as C
import os

import numpy as np

from . import ba_types as T
from . import synth_ba

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(_HERE, "lib", "libov2host.so"))
        dp, ip, u8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        L.ov2h_map_create.restype = C.c_void_p
        L.ov2h_map_create.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_int, C.c_int, C.c_int]
        L.ov2h_map_destroy.argtypes = [C.c_void_p]
        L.ov2h_map_add_keyframe.argtypes = [C.c_void_p, C.c_int, dp]
        L.ov2h_map_add_landmark.argtypes = [C.c_void_p, C.c_int, dp, C.c_int]
        L.ov2h_map_add_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
        L.ov2h_map_finalize.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_local_ba_setup.argtypes = [C.c_void_p, C.c_int, ip, ip, ip]
        L.ov2h_map_attach_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ov2h_local_ba_setup_dev.argtypes = [C.c_void_p, C.c_int, ip, ip, ip]
        L.ov2h_map_device_rows.argtypes = [C.c_void_p, ip, ip, ip]
        L.ov2h_map_device_handle.argtypes = [C.c_void_p]
        L.ov2h_map_device_handle.restype = C.c_void_p
        L.ov2h_map_flush_device.argtypes = [C.c_void_p]
        L.ov2h_set_distortion.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, dp]
        L.ov2h_undistort.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.ov2h_project_dist.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_float)]
        L.ov2h_range_ba_setup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, ip]
        L.ov2h_full_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, C.POINTER(C.c_double), ip]
        L.ov2h_local_pose_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, dp, C.POINTER(C.c_double), ip]
        L.ov2h_apply_local_pose_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp]
        L.ov2h_assemble_local_pose_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, C.c_int, ip, dp, u8, ip, ip, dp]
        L.ov2h_full_pose_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, dp, C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
        L.ov2h_loose_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_double)]
        L.ov2h_map_set_cur_frame.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_apply_loose_ba.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, C.c_int, u8, dp]
        L.ov2h_map_remove_keyframe.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_map_remove_obs.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ov2h_map_remove_landmark.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_map_set_isobs.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ov2h_map_bad_lmids.argtypes = [C.c_void_p, ip, C.c_int]
        fp = C.POINTER(C.c_float)
        L.ov2h_local_ba_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u8, ip, ip]
        L.ov2h_local_ba_update.argtypes = [C.c_void_p, C.c_int, C.c_int, u8, C.c_int]
        L.ov2h_map_add_keyframe_obs.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, ip, fp, u8, fp]
        L.ov2h_map_append_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, fp, u8, fp]
        L.ov2h_map_export.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, ip, dp, ip, dp, u8, ip, ip, u8]
        L.ov2h_local_ba_get.argtypes = [C.c_void_p, ip, u8, dp, ip, dp, ip, dp, u8, ip, ip, dp]
        L.ov2h_apply_local_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, dp]
        L.ov2h_ba_worker_create.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int]
        L.ov2h_ba_worker_create.restype = C.c_void_p
        L.ov2h_ba_worker_set_device_resident.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_ba_worker_set_device_resident.restype = None
        L.ov2h_ba_worker_submit_all.argtypes = [C.c_void_p]
        L.ov2h_ba_worker_submit_all.restype = None
        L.ov2h_ba_worker_set_counting.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_ba_worker_set_counting.restype = None
        L.ov2h_ba_worker_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_ba_worker_stats.restype = None
        L.ov2h_ba_worker_destroy.argtypes = [C.c_void_p]
        L.ov2h_ba_worker_destroy.restype = None
        L.ov2h_ba_pipeline_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, ip, dp, C.c_void_p, C.c_float, C.c_int, C.c_int]
        L.ov2h_slam_set_brief.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        L.ov2h_slam_set_brief.restype = None
        L.ov2h_slam_kf_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_slam_kf_stats.restype = None
        L.ov2h_slam_set_epipolar.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_ulonglong]
        L.ov2h_slam_set_epipolar.restype = None
        L.ov2h_slam_epi_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_slam_epi_stats.restype = None
        L.ov2h_slam_set_p3p.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_slam_set_p3p.restype = None
        L.ov2h_slam_p3p_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_slam_p3p_stats.restype = None
        L.ov2h_slam_set_temporal.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_slam_set_temporal.restype = None
        L.ov2h_slam_temporal_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_slam_temporal_stats.restype = None
        L.ov2h_map_add_kps.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, fp, u8, u8, dp]
        L.ov2h_map_forget_keyframe.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_map_forget_kp.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ov2h_triangulate_temporal.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, ip, ip, dp]
        L.ov2h_map_set_kp_stereo.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, fp]
        L.ov2h_map_set_right_cam.argtypes = [C.c_void_p, dp, dp, C.c_int]
        L.ov2h_triangulate_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, ip, ip, dp]
        L.ov2h_map_filtering.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, ip, dp]
        L.ov2h_map_export_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip]
        L.ov2h_slam_set_kf_filtering.argtypes = [C.c_void_p, C.c_float]
        L.ov2h_slam_set_kf_filtering.restype = None
        L.ov2h_slam_filter_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_slam_filter_stats.restype = None
        L.ov2h_landmark_invdepth.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_landmark_invdepth.restype = C.c_double
        L.ov2h_set_p3p.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_ulonglong]
        L.ov2h_p3p_stats.argtypes = [C.c_void_p, dp]
        L.ov2h_p3p_stats.restype = None
        L.ov2h_p3p_ransac.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_int, C.c_ulonglong, dp, ip, ip]
        L.ov2h_frame_counters.argtypes = [C.c_void_p, C.c_int, ip]
        L.ov2h_landmark_isobs.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_slam_device_handle.argtypes = [C.c_void_p]
        L.ov2h_slam_device_handle.restype = C.c_void_p
        L.ov2h_slam_flush_device.argtypes = [C.c_void_p]
        L.ov2h_slam_check_map.argtypes = [C.c_void_p, ip]
        L.ov2h_slam_export_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, ip, dp, ip, dp, u8, ip, ip, u8]
        L.ov2h_slam_export_map.restype = None
        L.ov2h_mp_new.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.ov2h_mp_new.restype = C.c_void_p
        L.ov2h_mp_add_obs.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_mp_add_obs.restype = None
        L.ov2h_mp_add_desc.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ov2h_mp_add_desc.restype = None
        L.ov2h_mp_remove_obs.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_mp_remove_obs.restype = None
        L.ov2h_mp_state.argtypes = [C.c_void_p, ip, u8, C.c_int, ip, C.POINTER(C.c_float)]
        L.ov2h_mp_free.argtypes = [C.c_void_p]
        L.ov2h_mp_free.restype = None
        L.ov2h_feloop_create.argtypes = [C.c_void_p, C.c_void_p]
        L.ov2h_feloop_create.restype = C.c_void_p
        L.ov2h_feloop_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, ip]
        L.ov2h_feloop_destroy.argtypes = [C.c_void_p]
        L.ov2h_feloop_destroy.restype = None
        L.ov2h_ba_pipeline_create.restype = C.c_void_p
        for fn in (L.ov2h_ba_pipeline_submit_all, L.ov2h_ba_pipeline_destroy):
            fn.argtypes, fn.restype = [C.c_void_p], None
        L.ov2h_ba_pipeline_set_counting.argtypes, L.ov2h_ba_pipeline_set_counting.restype = [C.c_void_p, C.c_int], None
        L.ov2h_ba_pipeline_stats.argtypes, L.ov2h_ba_pipeline_stats.restype = [C.c_void_p, dp], None
        L.ov2h_slam_create.argtypes = [C.c_void_p, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int]
        L.ov2h_slam_create.restype = C.c_void_p
        L.ov2h_slam_add_stereo.argtypes = [C.c_void_p, C.c_double, u8, u8, C.c_int, C.c_int]
        L.ov2h_slam_pose.argtypes, L.ov2h_slam_pose.restype = [C.c_void_p, dp], None
        L.ov2h_slam_stats.argtypes, L.ov2h_slam_stats.restype = [C.c_void_p, dp], None
        L.ov2h_slam_landmarks.argtypes = [C.c_void_p, C.c_int, ip, dp]
        L.ov2h_slam_destroy.argtypes, L.ov2h_slam_destroy.restype = [C.c_void_p], None
        L.ov2h_compute_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, ip]
        L.ov2h_epipolar_filtering.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_ulonglong,
                                              C.c_int, ip, dp]
        L.ov2h_compute5pt.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                      C.c_ulonglong, dp, dp, ip, ip]
        L.ov2h_epi_opt_stats.argtypes, L.ov2h_epi_opt_stats.restype = [C.c_void_p, ip], None
        L.ov2h_check_ready_for_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                C.c_ulonglong, C.c_int, ip, ip, dp]
        L.ov2h_compute5pt_opt.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_int, C.c_float, C.c_float, C.c_float,
                                          C.c_ulonglong, dp, dp, ip, ip, ip]
        L.ov2h_get_pose.argtypes = [C.c_void_p, C.c_int, dp]
        L.ov2h_get_landmark.argtypes = [C.c_void_p, C.c_int, dp, ip]
        L.ov2h_count_keypoints.argtypes = [C.c_void_p, C.c_int, ip, ip, ip]
        L.ov2h_structure_only_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, dp, ip]
        fpp = C.POINTER(C.c_float)
        L.ov2h_map_add_kp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, dp]
        L.ov2h_frame_init_grid.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ov2h_map_forget_landmark.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_set_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ov2h_stereo_matching.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u8, u8, C.c_int, C.c_int]
        L.ov2h_klt_tracking.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u8, u8, C.c_int, C.c_int, ip]
        L.ov2h_get_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, fpp, u8, u8, fpp]
        L.ov2h_get_frl.argtypes = [C.c_void_p, C.c_int, dp]
        L.ov2h_map_add_desc.argtypes = [C.c_void_p, C.c_int, C.c_int, u8]
        L.ov2h_map_set_covscore.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ov2h_loop_assemble.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, u8, u8]
        L.ov2h_loop_local_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, ip, ip, ip, ip]
        L.ov2h_loop_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, dp, C.c_float, C.c_float, ip, ip, C.c_int, ip, ip, ip, ip]
        L.ov2h_loop_compute_pnp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, C.c_int, ip, ip]
        ull = C.POINTER(C.c_ulonglong)
        L.ov2h_loop_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, ip, ip, ull, C.c_int, C.c_float, C.c_int, ip, dp, ip, ip]
        L.ov2h_loop_verify_candidate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.c_ulonglong, C.c_int, C.c_float,
                                                 C.c_int, ip, dp, ip]
        L.ov2h_loop_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, ull, C.c_int, C.c_float, C.c_int, ip, ip, ip, dp, ip, ip]
        L.ov2h_loop_accept.argtypes = [C.c_int, C.c_int]
        L.ov2h_loop_remove_outliers.argtypes = [C.c_int, ip, C.c_int, ip]
        L.ov2h_loop_candidate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_float, C.c_int, ip, ip, ip, ip]
        L.ov2h_loop_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip, ip, C.POINTER(C.c_ulonglong), C.c_int, C.c_float, C.c_int,
                                      ip, ip, ip, dp, ip, ip, ip]
        L.ov2h_match_assemble.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_int, ip, ip, ip]
        L.ov2h_match_local_maps.argtypes = [C.c_int, C.c_void_p, C.c_void_p, ip, ip, ip, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                            ip, ip, ip]
        L.ov2h_match_local_maps_mirror.argtypes = L.ov2h_match_local_maps.argtypes
        L.ov2h_map_enable_match_columns.argtypes = [C.c_void_p]
        L.ov2h_update_frame_covisibility.argtypes = [C.c_void_p, C.c_int]
        L.ov2h_extend_local_map.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ov2h_frame_local_ids.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip]
        L.ov2h_frame_set_local_ids.argtypes = [C.c_void_p, C.c_int, C.c_int, ip]
        L.ov2h_frame_cov_map.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, ip]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class HostMap:
    """a MapManager + keyframes + map points built from a flat BaProblem (inverse-depth or XYZ window)."""

    def __init__(self, prob, nmin_covscore=25, stereo=True):
        L = lib()
        self.prob = prob
        T_rl = np.eye(4)
        T_rl[:3, :3] = synth_ba.quat_to_rot(prob.T_rl[3:])
        T_rl[:3, 3] = prob.T_rl[:3]
        T_lr = np.linalg.inv(T_rl)
        t_lr7 = np.ascontiguousarray(synth_ba.pose7(T_lr[:3, :3], T_lr[:3, 3]))
        self.h = L.ov2h_map_create(int(stereo), prob.inv_depth, _dp(prob.calib_l), _dp(prob.calib_r), _dp(t_lr7), 752, 480,
                                   nmin_covscore)
        for k in range(len(prob.pose)):
            L.ov2h_map_add_keyframe(self.h, k, _dp(np.ascontiguousarray(prob.pose[k])))
        # observations per (kf, lm) from the residual list
        obs = {}
        for i in range(prob.n_res):
            t, k, l = int(prob.res_type[i]), int(prob.res_pose[i]), int(prob.res_lm[i])
            if t == T.RANCH_INV:
                k = int(prob.lm_anchor_pose[l])
            o = obs.setdefault((k, l), {})
            if t in (T.L_XYZ, T.L_INV):
                o["l"] = prob.res_uv[i]
            else:
                o["r"] = prob.res_uv[i]
        self.xyz0 = np.zeros((len(prob.lm), 3))
        for l in range(len(prob.lm)):
            if prob.inv_depth:
                a = int(prob.lm_anchor_pose[l])
                obs.setdefault((a, l), {})["l"] = prob.lm_anchor_uv[l]
                z = 1.0 / prob.lm[l, 0]
                u, v = prob.lm_anchor_uv[l]
                pc = z * np.array([(u - prob.calib_l[2]) / prob.calib_l[0], (v - prob.calib_l[3]) / prob.calib_l[1], 1.0])
                xyz = synth_ba.quat_to_rot(prob.pose[a, 3:]) @ pc + prob.pose[a, :3]
            else:
                xyz = prob.lm[l]
            self.xyz0[l] = xyz
        anchor = {}
        for (k, l) in obs:
            anchor[l] = min(anchor.get(l, 10 ** 9), k)
        for l in range(len(prob.lm)):
            if l in anchor:
                L.ov2h_map_add_landmark(self.h, l, _dp(np.ascontiguousarray(self.xyz0[l])), anchor[l])
        for (k, l), o in sorted(obs.items()):
            ul = o["l"]
            ur = o.get("r")
            L.ov2h_map_add_obs(self.h, k, l, ul[0], ul[1], int(ur is not None), 0.0 if ur is None else ur[0],
                               0.0 if ur is None else ur[1])
        self.newkf = len(prob.pose) - 1
        assert L.ov2h_map_finalize(self.h, self.newkf) == 0

    def __del__(self):
        if getattr(self, "h", None):
            lib().ov2h_map_destroy(self.h)
            self.h = None

    def attach_device(self, ctx, max_kf=None, max_lm=None, max_obs=None):
        """MapManager::attachDevice: mirror the whole map into an ov2_map (HBM tables); later set-ups can run there."""
        n_obs = self.prob.n_res + len(self.prob.lm)
        rc = lib().ov2h_map_attach_device(self.h, ctx.h, max_kf or len(self.prob.pose) + 8, max_lm or len(self.prob.lm) + 8,
                                          max_obs or n_obs + 64)
        if rc != 0:
            raise RuntimeError(f"attachDevice failed (status {rc})")

    def set_distortion(self, cam, model, coeffs):
        """CameraCalibration::Dcv_ of the left (0) / right (1) camera: model 'pinhole' (k1 k2 p1 p2 [k3]) or 'fisheye' (k1..k4)"""
        d = np.ascontiguousarray(coeffs, np.float64)
        assert lib().ov2h_set_distortion(self.h, int(cam), 1 if model == "fisheye" else 0, len(d), _dp(d)) == 0

    def undistort(self, cam, x, y):
        out = (C.c_float * 2)()
        assert lib().ov2h_undistort(self.h, int(cam), float(x), float(y), out) == 0
        return np.array([out[0], out[1]], np.float32)

    def project_dist(self, cam, pc):
        out = (C.c_float * 2)()
        assert lib().ov2h_project_dist(self.h, int(cam), _dp(np.ascontiguousarray(pc, np.float64)), out) == 0
        return np.array([out[0], out[1]], np.float32)

    def device_handle(self):
        """the ov2_map* of the attached device mirror"""
        return C.c_void_p(lib().ov2h_map_device_handle(self.h))

    def flush_device(self):
        assert lib().ov2h_map_flush_device(self.h) == 0

    def device_rows(self):
        """(rows, capacity, compactions) of the device mirror's observation table"""
        r, c, n = C.c_int(), C.c_int(), C.c_int()
        assert lib().ov2h_map_device_rows(self.h, C.byref(r), C.byref(c), C.byref(n)) == 0
        return r.value, c.value, n.value

    def remove_obs(self, kfid, lmid):
        lib().ov2h_map_remove_obs(self.h, int(kfid), int(lmid))

    def remove_landmark(self, lmid):
        lib().ov2h_map_remove_landmark(self.h, int(lmid))

    def set_isobs(self, lmid, isobs):
        """MapPoint::isobs_ (seen by the current frame)"""
        assert lib().ov2h_map_set_isobs(self.h, int(lmid), int(isobs)) == 0

    def bad_lmids(self):
        buf = np.zeros(max(1, len(self.prob.lm)), np.int32)
        n = lib().ov2h_map_bad_lmids(self.h, buf.ctypes.data_as(C.POINTER(C.c_int)), len(buf))
        return np.sort(buf[:n])

    def setup_local_ba(self, dev=False):
        """Optimizer::setupLocalBA (CPU hash-map walk) or, dev=True, Optimizer::setupLocalBADevice (scans of the device
        map mirror). returns dict of the flat problem keyed by reference ids."""
        L = lib()
        npose, nlm, nres = C.c_int(), C.c_int(), C.c_int()
        fn = L.ov2h_local_ba_setup_dev if dev else L.ov2h_local_ba_setup
        rc = fn(self.h, self.newkf, C.byref(npose), C.byref(nlm), C.byref(nres))
        if rc < 0:
            raise RuntimeError(f"local BA set-up failed ({rc})")
        self._n_res = nres.value
        return self._read_problem(rc, npose, nlm, nres)

    def setup_range_ba(self, kf_lo, kf_hi, kf_obs_max=2 ** 31 - 1, min_obs=0):
        """Optimizer::setupRangeBA: the set-up stage of fullBA (0, last, no observer filter, min_obs 3) / looseBA"""
        npose, nlm, nres = C.c_int(), C.c_int(), C.c_int()
        lib().ov2h_range_ba_setup(self.h, int(kf_lo), int(kf_hi), int(kf_obs_max), int(min_obs), C.byref(npose), C.byref(nlm), C.byref(nres))
        return self._read_problem(0, npose, nlm, nres)

    def full_ba(self, ctx, robust=True):
        """Optimizer::fullBA on the GPU. returns (status, outliers pass 1, pass 2, final cost, logged iterations)"""
        n1, n2, fc, it = C.c_int(), C.c_int(), C.c_double(), C.c_int()
        st = lib().ov2h_full_ba(self.h, ctx.h, int(robust), C.byref(n1), C.byref(n2), C.byref(fc), C.byref(it))
        return st, n1.value, n2.value, fc.value, it.value

    def loose_ba(self, ctx, inikfid, nkfid, robust=True):
        """Optimizer::looseBA on the GPU. returns (status, flagged observations, final cost)"""
        n1, fc = C.c_int(), C.c_double()
        st = lib().ov2h_loose_ba(self.h, ctx.h, int(inikfid), int(nkfid), int(robust), C.byref(n1), C.byref(fc))
        return st, n1.value, fc.value

    def remove_keyframe(self, kfid):
        """MapManager::removeKeyframe"""
        assert lib().ov2h_map_remove_keyframe(self.h, int(kfid)) == 0

    def update_frame_covisibility(self, kfid):
        """MapManager::updateFrameCovisibility on keyframe kfid (no GPU context): returns its Frame::map_covkfs_ as
        {covisible kfid: score}; the keyframe's local id set is updated by the store rule (local_ids reads it)"""
        L = lib()
        if L.ov2h_update_frame_covisibility(self.h, int(kfid)) != 0:
            raise RuntimeError(f"keyframe {kfid} is not in the map")
        ip, n = C.POINTER(C.c_int), C.c_int()
        assert L.ov2h_frame_cov_map(self.h, int(kfid), 0, None, None, C.byref(n)) == 0
        k, s = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32)
        assert L.ov2h_frame_cov_map(self.h, int(kfid), n.value, k.ctypes.data_as(ip), s.ctypes.data_as(ip), C.byref(n)) == 0
        return dict(zip(k[:n.value].tolist(), s[:n.value].tolist()))

    def extend_local_map(self, kfid, nmax_local):
        """the set assembly of Mapper::matchingToLocalMap on keyframe kfid (SlamManager::extendLocalMap, no GPU context):
        True when the extension branch was taken"""
        rc = lib().ov2h_extend_local_map(self.h, int(kfid), int(nmax_local))
        if rc < 0:
            raise RuntimeError(f"ov2h_extend_local_map: status {rc}")
        return bool(rc)

    def local_ids(self, kfid):
        """Frame::set_local_mapids_ of keyframe kfid, in its own iteration order"""
        L, ip, n = lib(), C.POINTER(C.c_int), C.c_int()
        if L.ov2h_frame_local_ids(self.h, int(kfid), 0, None, C.byref(n)) != 0:
            raise RuntimeError(f"keyframe {kfid} is not in the map")
        out = np.zeros(max(n.value, 1), np.int32)
        assert L.ov2h_frame_local_ids(self.h, int(kfid), n.value, out.ctypes.data_as(ip), C.byref(n)) == 0
        return out[:n.value].tolist()

    def set_local_ids(self, kfid, ids):
        """Frame::set_local_mapids_ of keyframe kfid becomes `ids`"""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if lib().ov2h_frame_set_local_ids(self.h, int(kfid), len(a), a.ctypes.data_as(C.POINTER(C.c_int))) != 0:
            raise RuntimeError(f"keyframe {kfid} is not in the map")

    def set_cur_frame(self, kfid):
        """MapManager::pcurframe_ becomes a Frame of its own with keyframe kfid's id, pose and keypoints (None: no current
        frame).  The constructor leaves the newest keyframe OBJECT as the current frame, which then receives the
        current-frame updates of looseBA / localPoseGraph on top of its keyframe update."""
        assert lib().ov2h_map_set_cur_frame(self.h, -1 if kfid is None else int(kfid)) == 0

    def apply_loose_ba(self, inikfid, nkfid, pose, lm, outlier):
        """Optimizer::applyLooseBA alone: looseBA's assembly, then the free poses (n_pose x 7), landmarks (n_lm x 1 or 3)
        and per-block flags (n_res bytes) replace those of the flat problem -- in the order setup_range_ba(inikfid, nkfid,
        kf_obs_max=nkfid, min_obs=0) lists them -- and the update stage runs.  Needs no GPU context; with a device mirror
        attached the edits wait in its dirty lists for flush_device().  returns T_corr = opt * inverse(old(nkfid)) as the
        stage formed it (7 doubles), or None when the range yields no residual block and nothing ran."""
        P = np.ascontiguousarray(pose, np.float64).reshape(-1, 7)
        Lm = np.ascontiguousarray(lm, np.float64)
        n_lm = Lm.shape[0] if Lm.ndim > 1 else (Lm.size if self.prob.inv_depth else Lm.size // 3)
        F = np.ascontiguousarray(outlier, np.uint8)
        T = np.zeros(7)
        rc = lib().ov2h_apply_loose_ba(self.h, int(inikfid), int(nkfid), len(P), _dp(P), int(n_lm), _dp(Lm), len(F),
                                       F.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(T))
        if rc < 0:
            raise RuntimeError(f"applyLooseBA failed ({rc})")
        return T if rc else None

    def local_pose_graph(self, ctx, newkf, kfloop_id, newTwc):
        """Optimizer::localPoseGraph. returns (1 accepted / 0 rejected, final cost, logged iterations)"""
        fc, nl = C.c_double(), C.c_int()
        T = np.ascontiguousarray(newTwc, np.float64)
        rc = lib().ov2h_local_pose_graph(self.h, ctx.h, int(newkf), int(kfloop_id), _dp(T), C.byref(fc), C.byref(nl))
        if rc < 0:
            raise RuntimeError(f"localPoseGraph failed ({rc})")
        return rc, fc.value, nl.value

    def assemble_local_pose_graph(self, newkf, kfloop_id, newTwc, cap=4096):
        """Optimizer::assembleLocalPoseGraph alone (no GPU context): None when there is no chain, else dict(kfids, pose (n x 7),
        pose_const, edge_i, edge_j, T_ij (n x 7)) -- the loop keyframe first, the closing edge last"""
        T = np.ascontiguousarray(newTwc, np.float64)
        ids, ei, ej = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        pose, Tij, cst = np.zeros((cap, 7)), np.zeros((cap, 7)), np.zeros(cap, np.uint8)
        ip = C.POINTER(C.c_int)
        n = lib().ov2h_assemble_local_pose_graph(self.h, int(newkf), int(kfloop_id), _dp(T), cap, ids.ctypes.data_as(ip), _dp(pose),
                                                 cst.ctypes.data_as(C.POINTER(C.c_uint8)), ei.ctypes.data_as(ip), ej.ctypes.data_as(ip),
                                                 _dp(Tij))
        if n < 0:
            raise RuntimeError(f"assembleLocalPoseGraph failed ({n})")
        if n == 0:
            return None
        return dict(kfids=ids[:n].copy(), pose=pose[:n].copy(), pose_const=cst[:n].copy(), edge_i=ei[:n].copy(), edge_j=ej[:n].copy(),
                    T_ij=Tij[:n].copy())

    def apply_local_pose_graph(self, newkf, kfids, Twc):
        """Optimizer::applyLocalPoseGraph alone: the free keyframes `kfids` (ascending, last = newkf) take the poses Twc
        (n x 7) as a solve would have left them, and keyframes / anchored landmarks / younger keyframes follow.  Needs no
        GPU context; with a device mirror attached the edits wait in its dirty lists for flush_device()."""
        k = np.ascontiguousarray(kfids, np.int32)
        T = np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
        assert len(k) == len(T)
        rc = lib().ov2h_apply_local_pose_graph(self.h, int(newkf), len(k), k.ctypes.data_as(C.POINTER(C.c_int)), _dp(T))
        if rc < 0:
            raise RuntimeError(f"applyLocalPoseGraph failed ({rc})")
        return rc

    def full_pose_graph(self, ctx, Twc, Tpc, iskf):
        """Optimizer::fullPoseGraph on (n x 7) poses, (n x 7) relative poses prev -> cur, keyframe flags. returns (ok, Twc, cost)"""
        Tw = np.ascontiguousarray(Twc, np.float64).copy()
        Tp = np.ascontiguousarray(Tpc, np.float64)
        kf = np.ascontiguousarray(iskf, np.uint8)
        fc = C.c_double()
        rc = lib().ov2h_full_pose_graph(self.h, ctx.h, len(Tw), _dp(Tw), _dp(Tp), kf.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(fc))
        if rc < 0:
            raise RuntimeError(f"fullPoseGraph failed ({rc})")
        return rc == 1, Tw, fc.value

    def _read_problem(self, rc, npose, nlm, nres):
        L = lib()
        e = 1 if self.prob.inv_depth else 3
        ip, u8 = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        out = dict(aborted=rc == 1, pose_kfid=np.zeros(npose.value, np.int32), pose_const=np.zeros(npose.value, np.uint8),
                   pose=np.zeros((npose.value, 7)), lm_lmid=np.zeros(nlm.value, np.int32), lm=np.zeros((nlm.value, e)),
                   lm_anchor_kfid=np.zeros(nlm.value, np.int32), lm_anchor_uv=np.zeros((nlm.value, 2)),
                   res_type=np.zeros(nres.value, np.uint8), res_kfid=np.zeros(nres.value, np.int32),
                   res_lmid=np.zeros(nres.value, np.int32), res_uv=np.zeros((nres.value, 2)))
        L.ov2h_local_ba_get(self.h, out["pose_kfid"].ctypes.data_as(ip), out["pose_const"].ctypes.data_as(u8), _dp(out["pose"]),
                            out["lm_lmid"].ctypes.data_as(ip), _dp(out["lm"]), out["lm_anchor_kfid"].ctypes.data_as(ip),
                            _dp(out["lm_anchor_uv"]), out["res_type"].ctypes.data_as(u8), out["res_kfid"].ctypes.data_as(ip),
                            out["res_lmid"].ctypes.data_as(ip), _dp(out["res_uv"]))
        return out

    # ---- Optimizer::localBA in its three stages, so that the map can be edited between set-up and update ----
    def solve_local_ba(self, ctx):
        """solves the problem of the last setup_local_ba() in place (Optimizer::localBA's host branch through ov2_ba_solve).
        returns (per residual block outlier flags in the set-up's order, outliers pass 1, pass 2)"""
        n = self._n_res
        out, n1, n2 = np.zeros(max(n, 1), np.uint8), C.c_int(), C.c_int()
        rc = lib().ov2h_local_ba_solve(self.h, ctx.h, self.newkf, out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n1), C.byref(n2))
        if rc != 0:
            raise RuntimeError(f"local BA solve failed ({rc})")
        return out[:n], n1.value, n2.value

    def update_local_ba(self, outlier, cur_frame_obs=True):
        """Optimizer::updateAfterLocalBA on the problem of the last setup_local_ba() (its states as set up or as
        solve_local_ba left them) with the given flags (set-up order), against the map as it is now (CPU only)"""
        f = np.ascontiguousarray(outlier, np.uint8)
        rc = lib().ov2h_local_ba_update(self.h, self.newkf, len(f), f.ctypes.data_as(C.POINTER(C.c_uint8)), int(bool(cur_frame_obs)))
        if rc != 0:
            raise RuntimeError(f"local BA update failed ({rc})")

    @staticmethod
    def _obs_args(lmid, uv, stereo, ruv):
        lmid = np.ascontiguousarray(lmid, np.int32)
        n = len(lmid)
        uv = np.ascontiguousarray(np.reshape(uv, (n, 2)), np.float32)
        stereo = np.ascontiguousarray(np.zeros(n) if stereo is None else stereo, np.uint8)
        ruv = np.ascontiguousarray(np.zeros((n, 2)) if ruv is None else np.reshape(ruv, (n, 2)), np.float32)
        fp = C.POINTER(C.c_float)
        return (n, lmid.ctypes.data_as(C.POINTER(C.c_int)), uv.ctypes.data_as(fp), stereo.ctypes.data_as(C.POINTER(C.c_uint8)),
                ruv.ctypes.data_as(fp), (lmid, uv, stereo, ruv))

    def add_keyframe_obs(self, kfid, Twc, lmid, uv, stereo=None, ruv=None):
        """MapManager::addKeyframe: a new keyframe observing existing landmarks (uv / ruv: undistorted pixels, float)"""
        n, pl, pu, ps, pr, _keep = self._obs_args(lmid, uv, stereo, ruv)
        T = np.ascontiguousarray(Twc, np.float64)
        assert lib().ov2h_map_add_keyframe_obs(self.h, int(kfid), _dp(T), n, pl, pu, ps, pr) == 0

    def append_obs(self, kfid, lmid, uv, stereo=None, ruv=None):
        """MapManager::addMapPointKfObs: observations joining an existing keyframe (the matchToMap / merge path)"""
        n, pl, pu, ps, pr, _keep = self._obs_args(lmid, uv, stereo, ruv)
        assert lib().ov2h_map_append_obs(self.h, int(kfid), n, pl, pu, ps, pr) == 0

    def export(self):
        """the whole map keyed by ids, as device_map.canonical_state gives a device map: ({kfid: pose}, {lmid: (xyz,
        OV2_LM_* state)}, {(kfid, lmid): stereo flag (0 / 2)}) of the live keyframes / landmarks / observations"""
        L, ip, u8 = lib(), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        n = np.zeros(3, np.int32)
        L.ov2h_map_export(self.h, 0, 0, 0, n.ctypes.data_as(ip), *([None] * 8))
        nk, nl, no = (int(v) for v in n)
        kid, kp, lid, lx = np.zeros(nk, np.int32), np.zeros((nk, 7)), np.zeros(nl, np.int32), np.zeros((nl, 3))
        ls, ok, ol, os_ = np.zeros(nl, np.uint8), np.zeros(no, np.int32), np.zeros(no, np.int32), np.zeros(no, np.uint8)
        L.ov2h_map_export(self.h, nk, nl, no, n.ctypes.data_as(ip), kid.ctypes.data_as(ip), _dp(kp), lid.ctypes.data_as(ip), _dp(lx),
                          ls.ctypes.data_as(u8), ok.ctypes.data_as(ip), ol.ctypes.data_as(ip), os_.ctypes.data_as(u8))
        kfs = {int(k): tuple(p) for k, p in zip(kid, kp)}
        lms = {int(l): (tuple(x), int(s)) for l, x, s in zip(lid, lx, ls)}
        obs = {(int(k), int(l)): 2 * int(s) for k, l, s in zip(ok, ol, os_)}
        return kfs, lms, obs

    def map_filtering(self, newkf=None, nmin_covscore=25, ratio=0.9, cap=4096):
        """Estimator::mapFiltering (src/estimator.cpp:101-183) with keyframe newkf as the new keyframe, on the host objects (no
        GPU context; an attached device mirror follows through MapManager::removeKeyframe).  Returns (removed kfids in removal
        order, dict(ran, candidates, few3d, unset3d))"""
        rm, st = np.zeros(cap, np.int32), np.zeros(4)
        n = lib().ov2h_map_filtering(self.h, int(self.newkf if newkf is None else newkf), int(nmin_covscore), float(ratio), cap,
                                     rm.ctypes.data_as(C.POINTER(C.c_int)), _dp(st))
        if n < 0:
            raise RuntimeError(f"mapFiltering: status {-1 - n}")
        return rm[:n].tolist(), dict(ran=int(st[0]), candidates=int(st[1]), few3d=int(st[2]), unset3d=int(st[3]))

    def export_graph(self):
        """the bookkeeping export() does not show: ({lmid: dict(kfid (anchor), is3d, isobs, observers: frozenset)},
        {kfid: {covisible kfid: count}} = Frame::map_covkfs_ of every keyframe)"""
        L, ip = lib(), C.POINTER(C.c_int)
        n = np.zeros(3, np.int32)
        L.ov2h_map_export_graph(self.h, 0, 0, 0, n.ctypes.data_as(ip), None, None, None)
        nl, no, nc = (int(v) for v in n)
        lm, ob, cv = np.zeros((nl, 4), np.int32), np.zeros((no, 2), np.int32), np.zeros((nc, 3), np.int32)
        L.ov2h_map_export_graph(self.h, nl, no, nc, n.ctypes.data_as(ip), lm.ctypes.data_as(ip), ob.ctypes.data_as(ip), cv.ctypes.data_as(ip))
        sets = {}
        for l, k in ob.tolist():
            sets.setdefault(l, set()).add(k)
        lms = {int(l): dict(kfid=int(a), is3d=bool(t), isobs=bool(o), observers=frozenset(sets.get(int(l), ()))) for l, a, t, o in lm.tolist()}
        kfs, _, _ = self.export()
        cov = {k: {} for k in kfs}
        for k, c, v in cv.tolist():
            cov[k][c] = v
        return lms, cov

    def apply_local_ba(self, ctx):
        """Estimator::applyLocalBA on the GPU. returns (status, outliers pass1, pass2, final cost)."""
        n1, n2, fc = C.c_int(), C.c_int(), C.c_double()
        st = lib().ov2h_apply_local_ba(self.h, ctx.h, self.newkf, C.byref(n1), C.byref(n2), C.byref(fc))
        return st, n1.value, n2.value, fc.value

    def compute_pose(self, ctx, kfid, Twc_init):
        """VisualFrontEnd::computePose with keyframe `kfid` as the current frame. returns (status, p3p requested)."""
        req = C.c_int()
        st = lib().ov2h_compute_pose(self.h, ctx.h, kfid, _dp(np.ascontiguousarray(Twc_init, np.float64)), C.byref(req))
        return st, bool(req.value)

    def set_p3p(self, dop3p=True, nransac_iter=100, fransac_err=3.0, bdo_random=False, seed=0):
        """dop3p / nransac_iter / fransac_err / bdo_random of the YAML for the P3P stage of computePose; seed = the sampler's
        base seed.  Clears a pending P3P request."""
        lib().ov2h_set_p3p(self.h, int(bool(dop3p)), int(nransac_iter), float(fransac_err), int(bool(bdo_random)),
                           int(seed) & ((1 << 64) - 1))

    def p3p_stats(self):
        """what the P3P branch did in the last compute_pose: dict(ran, status, points, removed, reset)"""
        e = np.zeros(5)
        lib().ov2h_p3p_stats(self.h, _dp(e))
        return dict(ran=int(e[0]), status=int(e[1]), points=int(e[2]), removed=int(e[3]), reset=int(e[4]))

    def structure_only_ba(self, ctx, lmids):
        """Optimizer::structureOnlyBA(vlm2optids) (src/optimizer.cpp:2594-2781). returns (status, final cost, LM iterations)"""
        ids = np.ascontiguousarray(lmids, np.int32)
        cost, it = C.c_double(0), C.c_int(0)
        st = lib().ov2h_structure_only_ba(self.h, ctx.h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cost), C.byref(it))
        return st, cost.value, it.value

    def pose(self, kfid):
        out = np.zeros(7)
        assert lib().ov2h_get_pose(self.h, kfid, _dp(out)) == 0
        return out

    def landmark(self, lmid):
        out, n = np.zeros(3), C.c_int()
        rc = lib().ov2h_get_landmark(self.h, lmid, _dp(out), C.byref(n))
        return (out, n.value) if rc == 0 else (None, 0)

    def counts(self, kfid):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib().ov2h_count_keypoints(self.h, kfid, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value


class EstimatorWorker:
    """the reference's Estimator thread (src/estimator.cpp:32-98) as a NATIVE thread of libov2host.so with its own
    high-priority HIP context: waits for keyframes and solves the windows of ALL sequences that have one pending in one
    ov2_ba_solve_batch call (at most max_batch).  Python only submits keyframes and reads the counters, so the worker never
    competes for the interpreter lock."""

    def __init__(self, device, problem, nseq, robust_mono_th=5.9915, max_batch=64, high_priority=True, device_resident=False):
        self.problem = problem              # keeps the arrays alive during the deep copy
        pc = problem.as_c()
        self.h = lib().ov2h_ba_worker_create(device, C.addressof(pc), robust_mono_th, nseq, max_batch, int(bool(high_priority)))
        if not self.h:
            raise RuntimeError("ov2h_ba_worker_create failed (no GPU?)")
        if device_resident:   # windows kept in HBM, solved by ov2_ba_solve_batch_dev (before the first submission)
            lib().ov2h_ba_worker_set_device_resident(self.h, 1)

    def submit_all(self):
        lib().ov2h_ba_worker_submit_all(self.h)

    def set_counting(self, on):
        lib().ov2h_ba_worker_set_counting(self.h, int(bool(on)))

    def stats(self):
        out = np.zeros(7)
        lib().ov2h_ba_worker_stats(self.h, _dp(out))
        return dict(solves=int(out[0]), iters=int(out[1]), dropped=int(out[2]), submitted=int(out[3]), busy_s=float(out[4]),
                    last_status=int(out[5]), batches=int(out[6]))

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_ba_worker_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class CppSlam:
    """ov2::SlamManager of libov2host.so (host/ov2_slam.hpp): the closed loop in C++ -- VisualFrontEnd::visualTracking per
    frame, MapManager::createKeyframe + Mapper::run + Estimator::applyLocalBA per keyframe -- driven one stereo frame per call.
    policy: None = the reference's own heuristics (checkNewKfReq, covisibility local BA, se3 motion model, its triangulation);
    'slam_loop' = the fixed stand-ins of ov2slam_amd.slam_loop.SlamLoop (keyframe every kf_every frames, BA over the last
    ba_window keyframes, ...), which makes the two loops comparable pose by pose."""

    STAT_KEYS = ("frame", "tracked", "n3d", "kf", "new_kps", "stereo", "n_lm", "ba", "ba_res", "ba_it_robust", "ba_it_l2",
                 "ba_outliers", "ba_cost0", "ba_cost1", "keyframes", "landmarks")

    def __init__(self, ctx, K4, baseline, w, h, cell=35, rectified=True, policy=None, kf_every=5, ba_window=8, ba_fixed=2,
                 device_map=False):
        pol = np.zeros(6, np.int32)
        if policy == "slam_loop":
            pol[:] = [kf_every, ba_window, ba_fixed, 1, 1, 1]
        elif policy is not None:
            raise ValueError(policy)
        K = np.ascontiguousarray(K4, np.float64)
        self.w, self.h, self.ctx = w, h, ctx
        self.h_ = lib().ov2h_slam_create(ctx.h, _dp(K), float(baseline), w, h, cell, int(bool(rectified)),
                                         pol.ctypes.data_as(C.POINTER(C.c_int)), int(bool(device_map)))
        if not self.h_:
            raise RuntimeError("ov2h_slam_create failed")
        self.traj, self.stats = [], []

    def step(self, time, img_left, img_right):
        u8 = C.POINTER(C.c_uint8)
        a, b = np.ascontiguousarray(img_left, np.uint8), np.ascontiguousarray(img_right, np.uint8)
        st = lib().ov2h_slam_add_stereo(self.h_, float(time), a.ctypes.data_as(u8), b.ctypes.data_as(u8), self.w, self.h)
        if st != 0:
            raise RuntimeError(f"SlamManager::addNewStereoImages failed ({st}): {self.ctx.lib.ov2_last_error(self.ctx.h)}")
        T, s = np.zeros(7), np.zeros(16)
        lib().ov2h_slam_pose(self.h_, _dp(T))
        lib().ov2h_slam_stats(self.h_, _dp(s))
        self.traj.append(T)
        self.stats.append(dict(zip(self.STAT_KEYS, s.tolist())))
        if getattr(self, "epi_stats", None) is not None:
            e = np.zeros(4)
            lib().ov2h_slam_epi_stats(self.h_, _dp(e))
            self.epi_stats.append(dict(status=int(e[0]), pairs=int(e[1]), removed=int(e[2]), gate_removed=int(e[3])))
        if getattr(self, "p3p_stats", None) is not None:
            e = np.zeros(5)
            lib().ov2h_slam_p3p_stats(self.h_, _dp(e))
            self.p3p_stats.append(dict(ran=int(e[0]), status=int(e[1]), points=int(e[2]), removed=int(e[3]), reset=int(e[4])))
        if getattr(self, "temporal_stats", None) is not None and self.stats[-1]["kf"]:
            e = np.zeros(5)
            lib().ov2h_slam_temporal_stats(self.h_, _dp(e))
            self.temporal_stats.append(dict(frame=int(self.stats[-1]["frame"]), ran=int(e[0]), kps2d=int(e[1]), candidates=int(e[2]),
                                            good=int(e[3]), removed=int(e[4])))
        if getattr(self, "filter_stats", None) is not None and self.stats[-1]["kf"]:
            e = np.zeros(16)
            lib().ov2h_slam_filter_stats(self.h_, _dp(e))
            self.filter_stats.append(dict(frame=int(self.stats[-1]["frame"]), ran=int(e[0]), candidates=int(e[1]), n_removed=int(e[2]),
                                          few3d=int(e[3]), unset3d=int(e[4]), removed=[int(k) for k in e[5:16] if k >= 0]))
        if getattr(self, "kf_stats", None) is not None and self.stats[-1]["kf"]:
            k = np.zeros(3)
            lib().ov2h_slam_kf_stats(self.h_, _dp(k))
            self.kf_stats.append(dict(frame=int(self.stats[-1]["frame"]), described=int(k[0]), local=int(k[1]), matched=int(k[2])))
        return T

    def set_brief(self, pattern, use_brief=True, track_localmap=True, fmax_desc_dist=0.0, fmax_proj_pxdist=0.0):
        """use_brief / bdo_track_localmap of the YAML: keyframes describe their keypoints (BRIEF-32 with the caller's 256 x 4 int8
        test table -- opencv_contrib's is not in the reference tree) and run Mapper::matchingToLocalMap + mergeMapPoints"""
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
        lib().ov2h_slam_set_brief(self.h_, None if pat is None else pat.ctypes.data, int(bool(use_brief)), int(bool(track_localmap)),
                                  float(fmax_desc_dist), float(fmax_proj_pxdist))
        self.kf_stats = []

    def set_epipolar(self, on=True, nransac_iter=100, fransac_err=3.0, bdo_random=True, seed=0):
        """doepipolar / nransac_iter / fransac_err / bdo_random of the YAML: trackMono runs VisualFrontEnd::epipolar2d2dFiltering
        (ov2_epipolar_filter_batch) between kltTracking and computePose; seed = the sampler's base seed"""
        lib().ov2h_slam_set_epipolar(self.h_, int(bool(on)), int(nransac_iter), float(fransac_err), int(bool(bdo_random)),
                                     int(seed) & ((1 << 64) - 1))
        self.epi_stats = []

    def set_p3p(self, dop3p=True):
        """dop3p of the YAML: computePose runs the P3P-LMedS bootstrap (ov2_p3p_ransac_batch) on every frame, not only when
        tracking asks for it; iterations, error bound and seed are those of set_epipolar.  Starts the per-frame p3p_stats list
        (also useful with dop3p off: the branch runs whenever bp3preq_ is set)."""
        lib().ov2h_slam_set_p3p(self.h_, int(bool(dop3p)))
        self.p3p_stats = []

    def set_kf_filtering(self, ratio=0.9):
        """kf_filtering_ratio of the YAML: Estimator::mapFiltering (src/estimator.cpp:101-183) culls redundant keyframes after
        every local BA.  1 is the reference's own 'off' and the default here; its parameter files set 0.9 or 0.95.  Starts the
        per-keyframe filter_stats list."""
        lib().ov2h_slam_set_kf_filtering(self.h_, float(ratio))
        self.filter_stats = []

    def set_temporal(self, on=True):
        """Mapper::triangulateTemporal in Mapper::run (src/mapper.cpp:107-126): the new keyframe's 2D keypoints are triangulated
        against the oldest keyframe that observes them.  The reference always runs it; here it is off until this call, because
        the existing loop tests hold counts recorded without it.  Starts the per-keyframe temporal_stats list."""
        lib().ov2h_slam_set_temporal(self.h_, int(bool(on)))
        self.temporal_stats = []

    def check_map(self):
        """(violations of the host map's invariants, total) -- see ov2h_slam_check_map"""
        v = np.zeros(6, np.int32)
        tot = lib().ov2h_slam_check_map(self.h_, v.ctypes.data_as(C.POINTER(C.c_int)))
        return dict(zip(("kp_without_mp", "kp_not_listed", "observer_without_kp", "covisibility", "mp3d_without_desc", "desc_without_observer"),
                        v.tolist())), int(tot)

    def export_map(self, cap_kf=4096, cap_lm=1 << 18, cap_obs=1 << 20):
        """the host map keyed by ids: ({kfid: pose}, {lmid: (xyz, state bits)}, {(kfid, lmid): stereo})"""
        ip, u8 = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        n = np.zeros(3, np.int32)
        kf_id, kf_pose = np.zeros(cap_kf, np.int32), np.zeros((cap_kf, 7))
        lm_id, lm_xyz, lm_st = np.zeros(cap_lm, np.int32), np.zeros((cap_lm, 3)), np.zeros(cap_lm, np.uint8)
        ok, ol, os_ = np.zeros(cap_obs, np.int32), np.zeros(cap_obs, np.int32), np.zeros(cap_obs, np.uint8)
        lib().ov2h_slam_export_map(self.h_, cap_kf, cap_lm, cap_obs, n.ctypes.data_as(ip), kf_id.ctypes.data_as(ip), _dp(kf_pose),
                                   lm_id.ctypes.data_as(ip), _dp(lm_xyz), lm_st.ctypes.data_as(u8), ok.ctypes.data_as(ip),
                                   ol.ctypes.data_as(ip), os_.ctypes.data_as(u8))
        assert n[0] <= cap_kf and n[1] <= cap_lm and n[2] <= cap_obs
        kfs = {int(k): tuple(p) for k, p in zip(kf_id[:n[0]], kf_pose[:n[0]])}
        lms = {int(l): (tuple(x), int(s)) for l, x, s in zip(lm_id[:n[1]], lm_xyz[:n[1]], lm_st[:n[1]])}
        obs = {(int(k), int(l)): int(s) for k, l, s in zip(ok[:n[2]], ol[:n[2]], os_[:n[2]])}
        return kfs, lms, obs

    def device_handle(self):
        return lib().ov2h_slam_device_handle(self.h_)

    def flush_device(self):
        st = lib().ov2h_slam_flush_device(self.h_)
        if st != 0:
            raise RuntimeError(f"MapManager::flushDevice failed ({st})")

    def landmarks(self, cap=1 << 16):
        ids, xyz = np.zeros(cap, np.int32), np.zeros((cap, 3))
        n = lib().ov2h_slam_landmarks(self.h_, cap, ids.ctypes.data_as(C.POINTER(C.c_int)), _dp(xyz))
        return ids[:n].copy(), xyz[:n].copy()

    def close(self):
        if getattr(self, "h_", None):
            lib().ov2h_slam_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        self.close()


class EstimatorPipeline:
    """the Estimator threads of `len(maps)` SLAM instances as ONE native thread that runs the WHOLE of Optimizer::localBA per
    keyframe job on device-resident maps (ov2slam_amd/device_map.DeviceMap, all created on `ctx`): set-up
    (ov2_map_local_ba_setup_batch, src/optimizer.cpp:43-430) -> solve (ov2_ba_solve_batch_dev, :439-735) -> update
    (ov2_map_local_ba_update_batch, :741-882) for every sequence that has a keyframe pending, in one batch.  `ctx` and the
    maps belong to the thread until close(); the caller must have saved the maps' state (every job starts from it)."""

    def __init__(self, ctx, maps, proto, robust_mono_th=5.9915, max_batch=64):
        self.ctx, self.maps, self.proto = ctx, maps, proto
        n = len(maps)
        hs = (C.c_void_p * n)(*[m.h for m in maps])
        nk = np.ascontiguousarray([m.newkf for m in maps], np.int32)
        K = np.ascontiguousarray(np.tile(np.asarray(proto.calib_l, np.float64), (n, 1)))
        pc = proto.as_c()
        self.h = lib().ov2h_ba_pipeline_create(ctx.h, n, hs, nk.ctypes.data_as(C.POINTER(C.c_int)), _dp(K), C.addressof(pc),
                                               robust_mono_th, int(proto.inv_depth), max_batch)
        if not self.h:
            raise RuntimeError("ov2h_ba_pipeline_create failed")

    def submit_all(self):
        lib().ov2h_ba_pipeline_submit_all(self.h)

    def set_counting(self, on):
        lib().ov2h_ba_pipeline_set_counting(self.h, int(bool(on)))

    def stats(self):
        o = np.zeros(40)
        lib().ov2h_ba_pipeline_stats(self.h, _dp(o))
        return dict(solves=int(o[0]), iters=int(o[1]), dropped=int(o[2]), submitted=int(o[3]), busy_s=float(o[4]),
                    last_status=int(o[5]), batches=int(o[6]), setup_s=float(o[7]), solve_s=float(o[8]), update_s=float(o[9]),
                    slowest_sum=int(o[10]), res_blocks=int(o[11]), aborted=int(o[12]), iter_blocks=int(o[13]),
                    hist_robust=[int(x) for x in o[16:24]], hist_l2=[int(x) for x in o[24:40]])

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_ba_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class _FeLoopCfg(C.Structure):   # ov2h_feloop_cfg (host/ov2_host_capi.cpp)
    _fields_ = [(k, C.c_int32) for k in ("L", "B", "n", "win", "nlvl", "use_clahe", "tiles_x", "tiles_y")] + \
               [(k, C.c_float) for k in ("clahe_clip", "err_th", "fb_th", "eps")] + \
               [(k, C.c_int32) for k in ("max_iter", "detect", "det_cell", "det_ncur", "det_cap", "pnp")] + \
               [(k, C.c_void_p) for k in ("left", "right", "kps", "pri", "st_pri", "has", "st_has", "img_idx", "out_xy", "out_st", "p3p",
                                          "pnp_off", "pnp_unpx", "pnp_wpts", "pnp_K", "pnp_T0", "pnp_T", "pnp_outl", "pnp_rem", "pnp_ok")] + \
               [("pnp_T_bytes", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("det_thresh", "det_cur", "det_img", "det_nout", "det_out")]


class FrameLoop:
    """native per-frame driver of a bench Workload (bench.py): the same sequence of ABI calls as Workload.step -- pyramid,
    kltTracking, ceresPnP; right pyramid, stereoMatching, detector and a job for every Estimator pipeline on keyframes --
    enqueued from C++ (ov2h_feloop_run), so that small streams are not bound by ~15 us of interpreter per call.  Holds
    references to the workload's device arrays; everything stays asynchronous."""

    def __init__(self, ctx, wl, win, nlvl, tiles, pipelines=()):
        self.ctx, self.wl = ctx, wl
        L = wl.L
        arr = lambda xs: (C.c_void_p * L)(*xs)
        self._keep = dict(left=arr([i.h_ for i in wl.left]), right=arr([i.h_ for i in wl.right]),
                          kps=arr([a.ptr for a in wl.kps]), pri=arr([a.ptr for a in wl.pri]), st_pri=arr([a.ptr for a in wl.st_pri]),
                          has=arr([a.ptr for a in wl.has]), st_has=arr([a.ptr for a in wl.st_has]))
        c = _FeLoopCfg()
        c.L, c.B, c.n, c.win, c.nlvl, c.use_clahe, c.tiles_x, c.tiles_y = L, wl.B, wl.n, win, nlvl, 1, tiles[0], tiles[1]
        c.clahe_clip, c.err_th, c.fb_th, c.eps, c.max_iter = 3.0, 30.0, 0.5, wl.trk.fmax_px_precision, wl.trk.nmax_iter
        c.detect, c.det_cell, c.det_ncur, c.det_cap = int(bool(wl.detect)), wl.det_cell, wl.det_ncur, wl.det_cap
        for k, v in self._keep.items():
            setattr(c, k, C.cast(v, C.c_void_p))
        c.img_idx, c.out_xy, c.out_st, c.p3p = wl.img_idx.ptr, wl.out_xy.ptr, wl.out_st.ptr, wl.p3p.ptr
        c.det_thresh, c.det_cur, c.det_img = wl.d_det_thresh.ptr, wl.d_det_cur.ptr, wl.d_det_img.ptr
        c.det_nout, c.det_out = wl.d_det_nout.ptr, wl.d_det_out.ptr
        if wl.pnp:
            q = wl.pnp
            c.pnp = 1
            c.pnp_off, c.pnp_unpx, c.pnp_wpts, c.pnp_K = q["off"].ptr, q["unpx"].ptr, q["wpts"].ptr, q["K"].ptr
            c.pnp_T0, c.pnp_T, c.pnp_T_bytes = q["T0"].ptr, q["T"].ptr, q["T"].nbytes
            c.pnp_outl, c.pnp_rem, c.pnp_ok = q["outl"].ptr, q["rem"].ptr, q["ok"].ptr
        self.cfg = c
        self.pipes = (C.c_void_p * max(1, len(pipelines)))(*[p.h for p in pipelines])
        self.n_pipes = len(pipelines)
        self.h = lib().ov2h_feloop_create(ctx.h, C.addressof(c))
        if not self.h:
            raise RuntimeError("ov2h_feloop_create failed")

    def run(self, steps, kf_every):
        """enqueue `steps` frames; returns the number of keyframes among them"""
        nk = C.c_int(0)
        st = lib().ov2h_feloop_run(self.h, int(steps), int(kf_every), self.pipes, self.n_pipes, C.byref(nk))
        if st != 0:
            raise RuntimeError(f"ov2h_feloop_run: status {st}: {self.ctx.lib.ov2_last_error(self.ctx.h).decode()}")
        return nk.value

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_feloop_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def compute5pt_essential(ctx, bvs1, bvs2, nmaxiter, errth, boptimize, fx, fy, seed):
    """the C++ MultiViewGeometry::compute5ptEssentialMatrix (src/multi_view_geometry.cpp:596-697) over the C ABI.
    returns (success, R (3,3), t (3,), voutliersidx); a negative status raises"""
    b1 = np.ascontiguousarray(bvs1, np.float64).reshape(-1, 3)
    b2 = np.ascontiguousarray(bvs2, np.float64).reshape(-1, 3)
    n = len(b1)
    R, t, out, nout = np.zeros(9), np.zeros(3), np.zeros(max(n, 1), np.int32), C.c_int(0)
    r = lib().ov2h_compute5pt(ctx.h, n, _dp(b1), _dp(b2), int(nmaxiter), float(errth), int(bool(boptimize)), float(fx), float(fy),
                              int(seed), _dp(R), _dp(t), out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nout))
    if r < 0:
        raise RuntimeError(f"compute5ptEssentialMatrix: status {r}")
    return bool(r), R.reshape(3, 3), t, out[:nout.value].copy()


def compute5pt_essential_opt(ctx, bvs1, bvs2, nmaxiter, errth, fx, fy, seed):
    """the C++ MultiViewGeometry::compute5ptEssentialMatrixOpt (the reference's call with do_optimize = true: RANSAC, then
    refine5pt on its inliers) over the C ABI.  returns (success, R (3,3), t (3,), voutliersidx, (refinement status, LM
    iterations)); a negative status raises"""
    b1 = np.ascontiguousarray(bvs1, np.float64).reshape(-1, 3)
    b2 = np.ascontiguousarray(bvs2, np.float64).reshape(-1, 3)
    n = len(b1)
    R, t, out, nout, ref = np.zeros(9), np.zeros(3), np.zeros(max(n, 1), np.int32), C.c_int(0), np.zeros(2, np.int32)
    ip = C.POINTER(C.c_int)
    r = lib().ov2h_compute5pt_opt(ctx.h, n, _dp(b1), _dp(b2), int(nmaxiter), float(errth), float(fx), float(fy), int(seed),
                                  _dp(R), _dp(t), out.ctypes.data_as(ip), C.byref(nout), ref.ctypes.data_as(ip))
    if r < 0:
        raise RuntimeError(f"compute5ptEssentialMatrixOpt: status {r}")
    return bool(r), R.reshape(3, 3), t, out[:nout.value].copy(), (int(ref[0]), int(ref[1]))


def p3p_ransac(ctx, bvs, vwpts, nmaxiter, errth, boptimize, bdorandom, fx, fy, Twc, use_lmeds=True, seed=0):
    """the C++ MultiViewGeometry::p3pRansac (src/multi_view_geometry.cpp:144-163) over the C ABI.
    returns (success, Twc (7,), voutliersidx); a negative status raises"""
    b, x = np.ascontiguousarray(bvs, np.float64).reshape(-1, 3), np.ascontiguousarray(vwpts, np.float64).reshape(-1, 3)
    n = len(b)
    T, out, nout = np.array(Twc, np.float64), np.zeros(max(n, 1), np.int32), C.c_int(0)
    r = lib().ov2h_p3p_ransac(ctx.h, n, _dp(b), _dp(x), int(nmaxiter), float(errth), int(bool(boptimize)), int(bool(bdorandom)),
                              float(fx), float(fy), int(bool(use_lmeds)), int(seed), _dp(T), out.ctypes.data_as(C.POINTER(C.c_int)),
                              C.byref(nout))
    if r < 0:
        raise RuntimeError(f"p3pRansac: status {r}")
    return bool(r), T, out[:nout.value].copy()


class TwoViewMap:
    """two keyframes of the C++ host mirror with chosen keypoints (pixels, 2D / 3D), to run
    VisualFrontEnd::epipolar2d2dFiltering with one as the previous keyframe and the other as the current frame"""

    def __init__(self, K, Twc_prev, Twc_cur, stereo=True, w=752, h=480):
        L = lib()
        K = np.ascontiguousarray(K, np.float64)
        t_lr7 = np.ascontiguousarray([0.11, 0, 0, 0, 0, 0, 1.0])
        self.h = L.ov2h_map_create(int(stereo), 1, _dp(K), _dp(K), _dp(t_lr7), w, h, 25)
        for kfid, T in ((0, Twc_prev), (1, Twc_cur)):
            L.ov2h_map_add_keyframe(self.h, kfid, _dp(np.ascontiguousarray(T, np.float64)))

    def add_keypoint(self, kfid, lmid, px, is3d):
        """kfid 0 = previous keyframe, 1 = current frame; px: undistorted pixel (float)"""
        x = np.zeros(3)
        assert lib().ov2h_map_add_kp(self.h, int(kfid), int(lmid), float(px[0]), float(px[1]), int(bool(is3d)), _dp(x)) == 0

    def epipolar_filtering(self, ctx, nransac_iter=100, fransac_err=3.0, seed=0, cap=1 << 16):
        """returns (removed ids ascending, stats dict); a negative status raises"""
        rm, st = np.zeros(cap, np.int32), np.zeros(4)
        n = lib().ov2h_epipolar_filtering(self.h, ctx.h, 0, 1, int(nransac_iter), float(fransac_err), int(seed), cap,
                                          rm.ctypes.data_as(C.POINTER(C.c_int)), _dp(st))
        if n < 0:
            raise RuntimeError(f"epipolar2d2dFiltering: status {n}")
        return rm[:n].copy(), dict(status=int(st[0]), pairs=int(st[1]), removed=int(st[2]), gate_removed=int(st[3]))

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class MonoMap(TwoViewMap):
    """a monocular map (stereo = 0 sets mono_) of the C++ host mirror: keyframes 0 .. N-1 at the given poses with chosen
    keypoints; the last one is taken as the current frame and the one before it as its keyframe, to run the mono branch of
    VisualFrontEnd::epipolar2d2dFiltering and VisualFrontEnd::checkReadyForInit"""

    def __init__(self, K, poses, w=752, h=480):
        L = lib()
        K = np.ascontiguousarray(K, np.float64)
        t_lr7 = np.ascontiguousarray([0.0, 0, 0, 0, 0, 0, 1.0])
        self.h = L.ov2h_map_create(0, 1, _dp(K), _dp(K), _dp(t_lr7), w, h, 25)
        self.nkf = len(poses)
        for kfid, T in enumerate(poses):
            L.ov2h_map_add_keyframe(self.h, kfid, _dp(np.ascontiguousarray(T, np.float64)))

    def _opt_stats(self, st):
        o = np.zeros(3, np.int32)
        lib().ov2h_epi_opt_stats(self.h, o.ctypes.data_as(C.POINTER(C.c_int)))
        return dict(status=int(st[0]), pairs=int(st[1]), removed=int(st[2]), gate_removed=int(st[3]), do_optimize=int(o[0]),
                    refine_status=int(o[1]), refine_iters=int(o[2]))

    def epipolar_filtering(self, ctx, nransac_iter=100, fransac_err=3.0, seed=0, cap=1 << 16):
        """returns (removed ids ascending, stats dict with the do_optimize fields); a negative status raises"""
        rm, st = np.zeros(cap, np.int32), np.zeros(4)
        n = lib().ov2h_epipolar_filtering(self.h, ctx.h, self.nkf - 2, self.nkf - 1, int(nransac_iter), float(fransac_err),
                                          int(seed), cap, rm.ctypes.data_as(C.POINTER(C.c_int)), _dp(st))
        if n < 0:
            raise RuntimeError(f"epipolar2d2dFiltering: status {n}")
        return rm[:n].copy(), self._opt_stats(st)

    def check_ready_for_init(self, ctx, finit_parallax=20.0, nransac_iter=100, fransac_err=3.0, seed=0, cap=1 << 16):
        """VisualFrontEnd::checkReadyForInit: returns (ready, removed ids ascending, stats dict); a negative status raises"""
        rm, st, n = np.zeros(cap, np.int32), np.zeros(4), C.c_int(0)
        r = lib().ov2h_check_ready_for_init(self.h, ctx.h, self.nkf - 2, self.nkf - 1, int(nransac_iter), float(fransac_err),
                                            float(finit_parallax), int(seed), cap, rm.ctypes.data_as(C.POINTER(C.c_int)),
                                            C.byref(n), _dp(st))
        if r < 0:
            raise RuntimeError(f"checkReadyForInit: status {r}")
        return bool(r), rm[:n.value].copy(), self._opt_stats(st)

    def pose(self, kfid=None):
        out = np.zeros(7)
        assert lib().ov2h_get_pose(self.h, self.nkf - 1 if kfid is None else int(kfid), _dp(out)) == 0
        return out


class TemporalMap(HostMap):
    """N keyframes of the C++ host mirror with 2D / 3D keypoints, built from a map of ov2slam_amd.synth_temporal.make_map, to
    run Mapper::triangulateTemporal (SlamManager::triangulateTemporal) on one of them.  export / attach_device / flush_device /
    device_handle are HostMap's."""

    def __init__(self, m, stereo=True):
        L = lib()
        K = np.ascontiguousarray(m["K4"], np.float64)
        t_lr7 = np.ascontiguousarray([0.11, 0, 0, 0, 0, 0, 1.0])
        self.h = L.ov2h_map_create(int(stereo), 1, _dp(K), _dp(K), _dp(t_lr7), int(m["w"]), int(m["h"]), 25)
        self.m, self.newkf = m, int(m["newkf"])
        ip, fp, u8 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        for k in range(m["n_kf"]):   # ascending: a map point is created by its oldest observer, as MapManager::addMapPoint does
            L.ov2h_map_add_keyframe(self.h, k, _dp(np.ascontiguousarray(m["poses"][k], np.float64)))
            sel = m["obs_kf"] == k
            lm = np.ascontiguousarray(m["obs_lm"][sel], np.int32)
            uv = np.ascontiguousarray(m["obs_uv"][sel], np.float32)
            kp3d, lm3d = np.ascontiguousarray(m["lm_kp3d"][lm], np.uint8), np.ascontiguousarray(m["lm_3d"][lm], np.uint8)
            xyz = np.ascontiguousarray(m["lm_xyz"][lm], np.float64)
            assert L.ov2h_map_add_kps(self.h, k, len(lm), lm.ctypes.data_as(ip), uv.ctypes.data_as(fp), kp3d.ctypes.data_as(u8),
                                      lm3d.ctypes.data_as(u8), _dp(xyz)) == 0
        for k, l in m["forget_kp"]:
            assert L.ov2h_map_forget_kp(self.h, int(k), int(l)) == 0
        for l in m["forget_lm"]:
            L.ov2h_map_forget_landmark(self.h, int(l))
        for k in m["forget_kf"]:
            L.ov2h_map_forget_keyframe(self.h, int(k))

    def attach_device(self, ctx, max_kf=None, max_lm=None, max_obs=None):
        rc = lib().ov2h_map_attach_device(self.h, ctx.h, max_kf or self.m["n_kf"] + 8, max_lm or self.m["n_lm"] + 8,
                                          max_obs or len(self.m["obs_kf"]) + 64)
        if rc != 0:
            raise RuntimeError(f"attachDevice failed (status {rc})")

    def triangulate_temporal(self, ctx, max_reproj_err=3.0):
        """the stage on keyframe newkf: (lmid ascending, ov2::TemporalBranch per keypoint, stats dict)"""
        cap = self.m["n_lm"]
        lm, br, st = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(4)
        ip = C.POINTER(C.c_int)
        n = lib().ov2h_triangulate_temporal(self.h, ctx.h, self.newkf, float(max_reproj_err), cap, lm.ctypes.data_as(ip),
                                            br.ctypes.data_as(ip), _dp(st))
        if n < 0:
            raise RuntimeError(f"triangulateTemporal: status {-1 - n}")
        return lm[:n].copy(), br[:n].copy(), dict(kps2d=int(st[0]), candidates=int(st[1]), good=int(st[2]), removed=int(st[3]))

    def invdepth(self, lmid):
        return float(lib().ov2h_landmark_invdepth(self.h, int(lmid)))


class StereoTriMap(TemporalMap):
    """the C++ host map of an ov2slam_amd.synth_stereo_tri.make_map dict -- keyframes with 2D / 3D keypoints, stereo keypoints
    with their right pixels (Frame::updateKeypointStereo), the right camera of the rig -- to run Mapper::triangulateStereo
    (SlamManager::triangulateStereo) on its new keyframe.  The dead rows and dead landmarks of the dict are not built."""

    def __init__(self, m, with_stereo=True):
        alive = (m["obs_alive"] != 0) & (m["lm_alive"][m["obs_lm"]] != 0)
        TemporalMap.__init__(self, dict(m, obs_kf=m["obs_kf"][alive], obs_lm=m["obs_lm"][alive], obs_uv=m["obs_uv"][alive],
                                        forget_kp=(), forget_lm=(), forget_kf=()), True)
        self.m = m
        assert lib().ov2h_map_set_right_cam(self.h, _dp(np.ascontiguousarray(m["Kr"], np.float64)),
                                            _dp(np.ascontiguousarray(m["Tlr"], np.float64)), int(m["rectified"])) == 0
        if with_stereo:
            st = alive & (m["obs_stereo"] != 0)
            for k in np.unique(m["obs_kf"][st]):
                sel = st & (m["obs_kf"] == k)
                self.set_kp_stereo(int(k), m["obs_lm"][sel], m["obs_rpx"][sel])

    def set_kp_stereo(self, kfid, lmid, rxy):
        """Frame::updateKeypointStereo(lmid[i], rxy[i]) on keyframe kfid (raw right pixels)"""
        lmid, rxy = np.ascontiguousarray(lmid, np.int32), np.ascontiguousarray(rxy, np.float32)
        assert lib().ov2h_map_set_kp_stereo(self.h, int(kfid), len(lmid), lmid.ctypes.data_as(C.POINTER(C.c_int)),
                                            rxy.ctypes.data_as(C.POINTER(C.c_float))) == 0

    def triangulate_stereo(self, ctx, max_reproj_err=3.0):
        """the stage on keyframe newkf: (lmid ascending, OV2_TRI_* verdict per keypoint, stats dict)"""
        cap = self.m["n_lm"]
        lm, vd, st = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(3)
        ip = C.POINTER(C.c_int)
        n = lib().ov2h_triangulate_stereo(self.h, ctx.h, self.newkf, float(max_reproj_err), cap, lm.ctypes.data_as(ip),
                                          vd.ctypes.data_as(ip), _dp(st))
        if n < 0:
            raise RuntimeError(f"triangulateStereo: status {-1 - n}")
        return lm[:n].copy(), vd[:n].copy(), dict(selected=int(st[0]), good=int(st[1]), demoted=int(st[2]))


class FilterMap(TemporalMap):
    """the C++ host map of a synth_filter.make_map dict -- keyframes, 2D / 3D keypoints, map points with their is3d_ / isobs_
    flags, covisibility counted by MapManager::updateFrameCovisibility -- to run Estimator::mapFiltering (map_filtering) on.
    Needs no GPU context unless a device mirror is attached."""

    def __init__(self, m, stereo=True):
        TemporalMap.__init__(self, dict(m, forget_kp=(), forget_lm=(), forget_kf=()), stereo)
        L = lib()
        for l in np.intersect1d(np.flatnonzero(m["lm_isobs"] == 0), m["obs_lm"]):   # map points are created observed
            assert L.ov2h_map_set_isobs(self.h, int(l), 0) == 0
        assert L.ov2h_map_finalize(self.h, self.newkf) == 0


class LoopMap:
    """the C++ host map of a synth_loop.make_scene dict -- keyframes with 2D / 3D keypoints, map points with one descriptor
    each (MapPoint::addDesc), chosen covisibility scores -- to run ov2::LoopCloser on: assemble (no GPU context), loop_match.
    A synth_revisit.make_local_map_scene dict adds world points, further descriptors per map point and the keypoint grid of
    the new keyframe: local_map (no GPU context), loop_track, compute_pnp."""

    def __init__(self, s):
        L = lib()
        K = np.ascontiguousarray(s["K4"], np.float64)
        t_lr7 = np.ascontiguousarray([0.11, 0, 0, 0, 0, 0, 1.0])
        self.h = L.ov2h_map_create(1, 1, _dp(K), _dp(K), _dp(t_lr7), int(s["w"]), int(s["h"]), 25)
        self.s = s
        ip, fp, u8 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        for k in s["kfids"]:
            L.ov2h_map_add_keyframe(self.h, int(k), _dp(np.ascontiguousarray(s["poses"][k], np.float64)))
            v = s["kps"][k]
            lm, uv = np.ascontiguousarray(v["lmid"], np.int32), np.ascontiguousarray(v["uv"], np.float32)
            kp3d = np.ascontiguousarray(v["kp3d"], np.uint8)
            lm3d = np.ascontiguousarray(v.get("lm3d", kp3d), np.uint8)   # MapPoint::is3d_ where it differs from the keypoint's flag
            xyz = np.ascontiguousarray(v["xyz"], np.float64) if "xyz" in v else np.zeros((len(lm), 3))   # world points, where the scene has them
            assert L.ov2h_map_add_kps(self.h, int(k), len(lm), lm.ctypes.data_as(ip), uv.ctypes.data_as(fp), kp3d.ctypes.data_as(u8),
                                      lm3d.ctypes.data_as(u8), _dp(xyz)) == 0
        for l, d in s["desc"].items():
            d = np.ascontiguousarray(d, np.uint8)
            kfid = min(k for k in s["kfids"] if l in s["kps"][k]["lmid"])
            assert L.ov2h_map_add_desc(self.h, int(l), int(kfid), d.ctypes.data_as(u8)) == 0
        for l, kd in s.get("descs", {}).items():      # further descriptors of a map point, one per observing keyframe, in this order
            for kfid, d in kd:
                d = np.ascontiguousarray(d, np.uint8)
                assert L.ov2h_map_add_desc(self.h, int(l), int(kfid), d.ctypes.data_as(u8)) == 0
        for k in s.get("grid_kfs", []):               # keyframes that need their keypoint grid (Frame::vgridkps_)
            assert L.ov2h_frame_init_grid(self.h, int(k), int(s["cell"])) == 0
        for l in s["forget_lm"]:
            L.ov2h_map_forget_landmark(self.h, int(l))
        for a, b, score in s["cov"]:
            assert L.ov2h_map_set_covscore(self.h, int(a), int(b), int(score)) == 0

    def attach_device(self, ctx, max_kf=None, max_lm=None, max_obs=None):
        """MapManager::attachDevice: mirror the whole map into an ov2_map"""
        s = self.s
        top = max(int(v["lmid"].max()) for v in s["kps"].values() if len(v["lmid"]))
        rc = lib().ov2h_map_attach_device(self.h, ctx.h, max_kf or max(s["kfids"]) + 9, max_lm or top + 9,
                                          max_obs or sum(len(v["lmid"]) for v in s["kps"].values()) + 64)
        if rc != 0:
            raise RuntimeError(f"attachDevice failed (status {rc})")

    def enable_match_columns(self):
        """MapManager::enableMatchColumns: the attached mirror keeps raw pixels and descriptors from here on"""
        rc = lib().ov2h_map_enable_match_columns(self.h)
        if rc != 0:
            raise RuntimeError(f"enableMatchColumns failed (status {rc})")

    def device_handle(self):
        """the ov2_map* of the attached device mirror"""
        return C.c_void_p(lib().ov2h_map_device_handle(self.h))

    def keypoint_order(self, kfid, cap=1 << 16):
        """lmids of keyframe kfid in the mirror's iteration order (Frame::getKeypoints)"""
        lm, px, a, b, rpx = np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), \
            np.zeros((cap, 2), np.float32)
        u8, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
        n = lib().ov2h_get_keypoints(self.h, int(kfid), cap, lm.ctypes.data_as(C.POINTER(C.c_int)), px.ctypes.data_as(fp),
                                     a.ctypes.data_as(u8), b.ctypes.data_as(u8), rpx.ctypes.data_as(fp))
        assert 0 <= n <= cap
        return lm[:n].tolist()

    def order(self):
        return {k: self.keypoint_order(k) for k in self.s["kfids"]}

    def assemble(self, newkf, lckf, cap=1 << 14):
        """what knnMatching hands to the matcher: (identity lmids, query lmids, train lmids, query rows, train rows)"""
        ip, u8 = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        n, q, t, i = np.zeros(3, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        qd, td = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
        rc = lib().ov2h_loop_assemble(self.h, int(newkf), int(lckf), cap, n.ctypes.data_as(ip), q.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                      i.ctypes.data_as(ip), qd.ctypes.data_as(u8), td.ctypes.data_as(u8))
        if rc != 0:
            raise RuntimeError(f"ov2h_loop_assemble: status {rc}")
        return i[:n[2]].tolist(), q[:n[0]].tolist(), t[:n[1]].tolist(), qd[:n[0]].copy(), td[:n[1]].copy()

    def local_map(self, newkf, lckf, vkplmids, cap=1 << 14):
        """what trackLoopLocalMap hands to its matcher (LoopCloser::assembleLoopLocalMap, no GPU context): dict(vkplmids: the
        list with the identity pairs appended, n_identity, matched: vmatchedkpids, local / cands: the local set and the
        candidates offered, in the mirror's order of first encounter)"""
        ip = C.POINTER(C.c_int)
        pin = np.ascontiguousarray(vkplmids, np.int32).reshape(-1, 2)
        n, po = np.zeros(4, np.int32), np.zeros((cap, 2), np.int32)
        m, lo, ca = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        rc = lib().ov2h_loop_local_map(self.h, int(newkf), int(lckf), len(pin), pin.ctypes.data_as(ip), cap, n.ctypes.data_as(ip),
                                       po.ctypes.data_as(ip), m.ctypes.data_as(ip), lo.ctypes.data_as(ip), ca.ctypes.data_as(ip))
        if rc < 0:
            raise RuntimeError(f"ov2h_loop_local_map: status {rc}")
        return dict(vkplmids=[tuple(r) for r in po[:n[0]].tolist()], n_identity=int(rc), matched=m[:n[1]].tolist(),
                    local=lo[:n[2]].tolist(), cands=ca[:n[3]].tolist())

    def loop_track(self, ctx, jobs, maxdist=10.0, ratio=0.3, cap=1 << 16):
        """LoopCloser::trackLoopLocalMaps: jobs = [(newkf, lckf, Twc (7,), vkplmids)]; returns (list of dict(vkplmids,
        n_identity, n_offered, n_matched), stats dict); a negative status raises"""
        B = len(jobs)
        ip = C.POINTER(C.c_int)
        nk = np.ascontiguousarray([j[0] for j in jobs], np.int32)
        lc = np.ascontiguousarray([j[1] for j in jobs], np.int32)
        T = np.ascontiguousarray([j[2] for j in jobs], np.float64).reshape(-1, 7)
        n_in = np.ascontiguousarray([len(j[3]) for j in jobs], np.int32)
        pin = np.ascontiguousarray([p for j in jobs for p in j[3]], np.int32).reshape(-1, 2)
        n_out, po, cnt, st = np.zeros(max(B, 1), np.int32), np.zeros((cap, 2), np.int32), np.zeros((max(B, 1), 3), np.int32), np.zeros(3, np.int32)
        rc = lib().ov2h_loop_track(self.h, ctx.h, B, nk.ctypes.data_as(ip), lc.ctypes.data_as(ip), _dp(T), float(maxdist), float(ratio),
                                   n_in.ctypes.data_as(ip), pin.ctypes.data_as(ip), cap, n_out.ctypes.data_as(ip), po.ctypes.data_as(ip),
                                   cnt.ctypes.data_as(ip), st.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"trackLoopLocalMaps: status {rc}")
        out, o = [], 0
        for b in range(B):
            out.append(dict(vkplmids=[tuple(r) for r in po[o:o + n_out[b]].tolist()], n_identity=int(cnt[b, 0]), n_offered=int(cnt[b, 1]),
                            n_matched=int(cnt[b, 2])))
            o += n_out[b]
        return out, dict(pairs=int(st[0]), match_pairs=int(st[1]), match_calls=int(st[2]))

    def compute_pnp(self, ctx, kfid, vkplmids, Twc, voutlier_idx=(), cap=1 << 14):
        """LoopCloser::computePnP: returns (success, Twc (7,), voutlier_idx: the given indices followed by the appended ones);
        a negative status raises"""
        ip = C.POINTER(C.c_int)
        pin = np.ascontiguousarray(vkplmids, np.int32).reshape(-1, 2)
        T, out, nout = np.array(Twc, np.float64), np.zeros(cap, np.int32), C.c_int(0)
        out[:len(voutlier_idx)] = list(voutlier_idx)
        rc = lib().ov2h_loop_compute_pnp(self.h, ctx.h, int(kfid), len(pin), pin.ctypes.data_as(ip), _dp(T), len(voutlier_idx), cap,
                                         out.ctypes.data_as(ip), C.byref(nout))
        if rc < 0:
            raise RuntimeError(f"computePnP: status {rc}")
        return bool(rc), T, out[:nout.value].tolist()

    VERIFY_STATS = ("p3p_pairs", "refine_pairs", "track_pairs", "pnp_pairs", "p3p_calls", "refine_calls", "track_calls", "pnp_calls")

    @staticmethod
    def _unpack_verify(B, ints, dbl, lists):
        """the rows ov2h_loop_verify writes -> list of dicts (no arithmetic: slicing only)"""
        out, o = [], 0
        for b in range(B):
            i, d = ints[b].tolist(), dbl[b]
            take = []
            for n, w in ((i[6], 2), (i[7], 2), (i[8], 2), (i[12], 1)):
                take.append(lists[o:o + n * w].reshape(-1, w).tolist())
                o += n * w
            out.append(dict(branch=i[0], p3p_status=i[1], p3p_info=i[2:6], after_p3p=[tuple(r) for r in take[0]],
                            after_track=[tuple(r) for r in take[1]], final=[tuple(r) for r in take[2]], pnp_outliers=[r[0] for r in take[3]],
                            n_identity=i[9], n_offered=i[10], n_matched=i[11], Twc_p3p=d[:7].copy(), Twc=d[7:14].copy(),
                            lc_pose_err=float(d[14])))
        return out

    def loop_verify(self, ctx, pairs, lists, seeds, nransac_iter=100, fransac_err=3.0, cap=1 << 18):
        """LoopCloser::verifyLoopCandidates: pairs [(newkf, lckf)], lists: the incoming vkplmids of each, seeds; returns (list of
        per-pair dicts, stats dict); a negative status raises"""
        B = len(pairs)
        ip = C.POINTER(C.c_int)
        nk, lc = np.ascontiguousarray([p[0] for p in pairs], np.int32), np.ascontiguousarray([p[1] for p in pairs], np.int32)
        n_in = np.ascontiguousarray([len(v) for v in lists], np.int32)
        pin = np.ascontiguousarray([q for v in lists for q in v], np.int32).reshape(-1, 2)
        sd = np.ascontiguousarray(seeds, np.uint64)
        ints, dbl, li, st = np.zeros((max(B, 1), 13), np.int32), np.zeros((max(B, 1), 15)), np.zeros(cap, np.int32), np.zeros(8, np.int32)
        rc = lib().ov2h_loop_verify(self.h, ctx.h, B, nk.ctypes.data_as(ip), lc.ctypes.data_as(ip), n_in.ctypes.data_as(ip),
                                    pin.ctypes.data_as(ip), sd.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(nransac_iter),
                                    float(fransac_err), cap, ints.ctypes.data_as(ip), _dp(dbl), li.ctypes.data_as(ip), st.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"verifyLoopCandidates: status {rc}")
        return self._unpack_verify(B, ints, dbl, li), dict(zip(self.VERIFY_STATS, st.tolist()))

    def loop_verify_candidate(self, ctx, newkf, lckf, vkplmids, seed, nransac_iter=100, fransac_err=3.0, cap=1 << 16):
        """LoopCloser::verifyLoopCandidate, the reference-shaped call on one pair: one dict as loop_verify returns them"""
        ip = C.POINTER(C.c_int)
        pin = np.ascontiguousarray(vkplmids, np.int32).reshape(-1, 2)
        ints, dbl, li = np.zeros((1, 13), np.int32), np.zeros((1, 15)), np.zeros(cap, np.int32)
        rc = lib().ov2h_loop_verify_candidate(self.h, ctx.h, int(newkf), int(lckf), len(pin), pin.ctypes.data_as(ip), int(seed),
                                              int(nransac_iter), float(fransac_err), cap, ints.ctypes.data_as(ip), _dp(dbl),
                                              li.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"verifyLoopCandidate: status {rc}")
        return self._unpack_verify(1, ints, dbl, li)[0]

    def loop_process(self, ctx, pairs, seeds, nransac_iter=100, fransac_err=3.0, cap=1 << 18):
        """LoopCloser::processLoopCandidates: (branches of the 2D-2D half, pairs each passed on, per-pair verify dicts, stats)"""
        B = len(pairs)
        ip = C.POINTER(C.c_int)
        nk, lc = np.ascontiguousarray([p[0] for p in pairs], np.int32), np.ascontiguousarray([p[1] for p in pairs], np.int32)
        sd = np.ascontiguousarray(seeds, np.uint64)
        br, npass = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        ints, dbl, li, st = np.zeros((max(B, 1), 13), np.int32), np.zeros((max(B, 1), 15)), np.zeros(cap, np.int32), np.zeros(13, np.int32)
        rc = lib().ov2h_loop_process(self.h, ctx.h, B, nk.ctypes.data_as(ip), lc.ctypes.data_as(ip), sd.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                     int(nransac_iter), float(fransac_err), cap, br.ctypes.data_as(ip), npass.ctypes.data_as(ip),
                                     ints.ctypes.data_as(ip), _dp(dbl), li.ctypes.data_as(ip), st.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"processLoopCandidates: status {rc}")
        keys = ("pairs", "knn_pairs", "epi_pairs", "knn_calls", "epi_calls") + self.VERIFY_STATS
        return br[:B].tolist(), npass[:B].tolist(), self._unpack_verify(B, ints, dbl, li), dict(zip(keys, st.tolist()))

    def loop_candidate(self, ctx, newkf, lckf, seed, nransac_iter=100, fransac_err=3.0, cap=1 << 14):
        """LoopCloser::processLoopCandidate as the reference writes it, one pair: dict(branch, lckfid, knn, n_outliers, out,
        success: the filter's bool, -1 = not reached); a negative status raises"""
        ip = C.POINTER(C.c_int)
        o, ok, pk, po = np.zeros(5, np.int32), C.c_int(-1), np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.int32)
        rc = lib().ov2h_loop_candidate(self.h, ctx.h, int(newkf), int(lckf), int(seed), int(nransac_iter), float(fransac_err), cap,
                                       o.ctypes.data_as(ip), C.byref(ok), pk.ctypes.data_as(ip), po.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"processLoopCandidate: status {rc}")
        return dict(branch=int(o[0]), lckfid=int(o[1]), knn=[tuple(r) for r in pk[:o[2]].tolist()], n_outliers=int(o[3]),
                    out=[tuple(r) for r in po[:o[4]].tolist()], success=ok.value)

    def loop_match(self, ctx, pairs, seeds, nransac_iter=100, fransac_err=3.0, cap=1 << 16):
        """LoopCloser::matchLoopCandidates: (list of per-pair dicts, stats dict); a negative status raises"""
        B = len(pairs)
        ip = C.POINTER(C.c_int)
        nk = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        lc = np.ascontiguousarray([p[1] for p in pairs], np.int32)
        sd = np.ascontiguousarray(seeds, np.uint64)
        branch, counts, info, Rt = np.zeros(B, np.int32), np.zeros((B, 8), np.int32), np.zeros((B, 4), np.int32), np.zeros((B, 12))
        pk, po, stats = np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.int32), np.zeros(5, np.int32)
        rc = lib().ov2h_loop_match(self.h, ctx.h, B, nk.ctypes.data_as(ip), lc.ctypes.data_as(ip), sd.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                   int(nransac_iter), float(fransac_err), cap, branch.ctypes.data_as(ip), counts.ctypes.data_as(ip),
                                   info.ctypes.data_as(ip), _dp(Rt), pk.ctypes.data_as(ip), po.ctypes.data_as(ip), stats.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"matchLoopCandidates: status {rc}")
        out, ok, oo = [], 0, 0
        for b in range(B):
            c = counts[b]
            out.append(dict(branch=int(branch[b]), lckfid=int(c[0]), n_identity=int(c[1]), n_query=int(c[2]), n_train=int(c[3]),
                            knn=[tuple(r) for r in pk[ok:ok + c[4]].tolist()], n_outliers=int(c[5]),
                            out=[tuple(r) for r in po[oo:oo + c[6]].tolist()], status=int(c[7]), info=info[b].tolist(),
                            R=Rt[b, :9].copy(), t=Rt[b, 9:].copy()))
            ok += c[4]
            oo += c[6]
        return out, dict(pairs=int(stats[0]), knn_pairs=int(stats[1]), epi_pairs=int(stats[2]), knn_calls=int(stats[3]),
                         epi_calls=int(stats[4]))

    # the steps of the chain one by one, and what a test reads back: HostMap's methods work on any ov2h map handle
    local_pose_graph = HostMap.local_pose_graph
    structure_only_ba = HostMap.structure_only_ba
    loose_ba = HostMap.loose_ba
    pose = HostMap.pose
    landmark = HostMap.landmark
    remove_obs = HostMap.remove_obs
    remove_landmark = HostMap.remove_landmark
    remove_keyframe = HostMap.remove_keyframe
    update_frame_covisibility = HostMap.update_frame_covisibility
    extend_local_map = HostMap.extend_local_map
    local_ids = HostMap.local_ids
    set_local_ids = HostMap.set_local_ids

    def merge_points(self, prevlmid, newlmid):
        """MapManager::mergeMapPoints"""
        L = lib()
        L.ov2h_map_merge_points.argtypes = [C.c_void_p, C.c_int, C.c_int]
        assert L.ov2h_map_merge_points(self.h, int(prevlmid), int(newlmid)) == 0

    def loop_close(self, ctx, newkf, lckf, Twc, vkplmids, cap=1 << 14):
        """LoopCloser::closeLoop on an accepted loop (src/loop_closer.cpp:302-372): dict as unpack_close gives it; a negative
        status raises"""
        return loop_close_batch(ctx, [self], [newkf], [lckf], [Twc], [vkplmids], cap, single=True)[0]

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


LCL_FEW_PAIRS, LCL_PG_REFUSED, LCL_CLOSED, LCL_CLOSED_LOOSE_BA = range(4)   # ov2::LoopCloseBranch
LCL_NOT_CALLED = 1                                                          # a status field whose call was not made


def unpack_close(ints, dbl, merged, stats):
    """one row of ov2h_loop_close -> dict (slicing only)"""
    i = [int(v) for v in ints]
    return dict(branch=i[0], inikfid=i[1], loose_start=i[2], pg_status=i[3], sba_status=i[4], loose_status=i[5],
                merged=[int(v) for v in merged[:i[6]]], pg_termination=i[7], pg_n_log=i[8], lc_pose_err=float(dbl[0]),
                pg_initial_cost=float(dbl[1]), pg_final_cost=float(dbl[2]),
                last_close=dict(jobs=int(stats[0]), graphs=int(stats[1]), solve_calls=int(stats[2])))


def loop_close_batch(ctx, maps, newkf, lckf, Twc, lists, cap=1 << 14, single=False):
    """LoopCloser::closeLoops on B LoopMaps of one context, one accepted loop each (Twc[b], lists[b] = its vkplmids): ONE
    pose-graph solve call for all, then apply / merge / structureOnlyBA / looseBA per map.  Returns the list of per-map dicts
    (each carries the call's last_close counts).  single: LoopCloser::closeLoop through its own hook (B must be 1)"""
    L, B = lib(), len(maps)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    nk, lc = np.ascontiguousarray(newkf, np.int32), np.ascontiguousarray(lckf, np.int32)
    T = np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
    n_in = np.ascontiguousarray([len(v) for v in lists], np.int32)
    pin = np.ascontiguousarray([q for v in lists for q in v], np.int32).reshape(-1, 2)
    ints, dbl = np.zeros((max(B, 1), 9), np.int32), np.zeros((max(B, 1), 3))
    merged, st = np.zeros((max(B, 1), cap), np.int32), np.zeros(3, np.int32)
    if single:
        assert B == 1
        L.ov2h_loop_close.argtypes = [vp, vp, C.c_int, C.c_int, dp, C.c_int, ip, C.c_int, ip, dp, ip, ip]
        rc = L.ov2h_loop_close(maps[0].h, ctx.h, int(nk[0]), int(lc[0]), _dp(T), int(n_in[0]), pin.ctypes.data_as(ip), cap,
                               ints.ctypes.data_as(ip), _dp(dbl), merged.ctypes.data_as(ip), st.ctypes.data_as(ip))
    else:
        L.ov2h_loop_close_batch.argtypes = [C.c_int, vp, vp, ip, ip, dp, ip, ip, C.c_int, ip, dp, ip, ip]
        hs = (vp * max(B, 1))(*[m.h for m in maps])
        rc = L.ov2h_loop_close_batch(B, hs, ctx.h, nk.ctypes.data_as(ip), lc.ctypes.data_as(ip), _dp(T), n_in.ctypes.data_as(ip),
                                     pin.ctypes.data_as(ip), cap, ints.ctypes.data_as(ip), _dp(dbl), merged.ctypes.data_as(ip),
                                     st.ctypes.data_as(ip))
    if rc != 0:
        raise RuntimeError(f"closeLoops: status {rc}")
    return [unpack_close(ints[b], dbl[b], merged[b], st) for b in range(B)]


def match_assemble(m, kfid, local, cap=1 << 14):
    """what Mapper::matchToMap hands to its matcher for keyframe kfid of the LoopMap m and the local lmid list `local`
    (SlamManager::assembleMatchToMap, no GPU context): (keypoint lmids in grid order, candidate lmids in the order offered)"""
    ip = C.POINTER(C.c_int)
    lo = np.ascontiguousarray(local, np.int32)
    n, kp, ca = np.zeros(2, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    rc = lib().ov2h_match_assemble(m.h, int(kfid), len(lo), lo.ctypes.data_as(ip), cap, n.ctypes.data_as(ip), kp.ctypes.data_as(ip),
                                   ca.ctypes.data_as(ip))
    if rc != 0:
        raise RuntimeError(f"ov2h_match_assemble: status {rc}")
    return kp[:n[0]].tolist(), ca[:n[1]].tolist()


MATCH_STATS = ("jobs", "match_jobs", "n_kp", "n_cand", "match_calls")


def match_local_maps(ctx, maps, kfids, locals, fmaxprojerr=2.0, fdistratio=0.2, merge=False, single=False, cap=1 << 16, mirror=False):
    """SlamManager::matchToLocalMaps on B LoopMaps of one context: keyframe kfids[b] of maps[b] re-matched against the lmid list
    locals[b] (Mapper::matchToMap) with ONE ov2_match_to_map_batch call for all; merge: MapManager::mergeMapPoints per pair
    afterwards (Mapper::mergeMatches); single: the same jobs as one ov2_match_to_map call each.  Returns (per-job lists of
    (previous lmid, new lmid) in ascending previous lmid, stats dict); a negative status raises"""
    L, B = lib(), len(maps)
    ip = C.POINTER(C.c_int)
    kf = np.ascontiguousarray(kfids, np.int32)
    n_local = np.ascontiguousarray([len(v) for v in locals], np.int32)
    lo = np.ascontiguousarray([l for v in locals for l in v], np.int32)
    n_pairs, pairs, st = np.zeros(max(B, 1), np.int32), np.zeros((cap, 2), np.int32), np.zeros(5, np.int32)
    hs = (C.c_void_p * max(B, 1))(*[m.h for m in maps])
    # mirror: ONE ov2_map_match_local_batch call on the maps' device mirrors instead, taken when every map has the match columns
    rc = (L.ov2h_match_local_maps_mirror if mirror else L.ov2h_match_local_maps)(B, hs, ctx.h, kf.ctypes.data_as(ip), n_local.ctypes.data_as(ip), lo.ctypes.data_as(ip), float(fmaxprojerr),
                                 float(fdistratio), int(bool(merge)), int(bool(single)), cap, n_pairs.ctypes.data_as(ip),
                                 pairs.ctypes.data_as(ip), st.ctypes.data_as(ip))
    if rc != 0:
        raise RuntimeError(f"matchToLocalMaps: status {rc}")
    out, o = [], 0
    for b in range(B):
        out.append([tuple(r) for r in pairs[o:o + n_pairs[b]].tolist()])
        o += n_pairs[b]
    return out, dict(zip(MATCH_STATS, st.tolist()))


class FrontEndFrame:
    """one keyframe with 2D / 3D keypoints in the C++ host mirror (Frame + MapManager + CameraCalibration pair), to drive
    MapManager::stereoMatching and VisualFrontEnd::kltTracking through libov2host.so.  Test / bring-up only."""

    def __init__(self, K, baseline, w, h, Twc=None, ncellsize=35, stereo_rect=False, klt_use_prior=True, nklt_pyr_lvl=3,
                 nklt_win_size=9):
        L = lib()
        K = np.ascontiguousarray(K, np.float64)
        t_lr7 = np.ascontiguousarray([baseline, 0, 0, 0, 0, 0, 1.0])    # right camera in the left frame (Tc0ci)
        self.h = L.ov2h_map_create(1, 1, _dp(K), _dp(K), _dp(t_lr7), w, h, 25)
        self.w, self.h_img, self.kfid = w, h, 0
        T = np.ascontiguousarray([0, 0, 0, 0, 0, 0, 1.0] if Twc is None else Twc, np.float64)
        L.ov2h_map_add_keyframe(self.h, 0, _dp(T))
        L.ov2h_set_params(self.h, int(klt_use_prior), int(stereo_rect), nklt_pyr_lvl, nklt_win_size)
        L.ov2h_frame_init_grid(self.h, 0, ncellsize)

    def add_keypoint(self, lmid, px, xyz=None):
        x = None if xyz is None else np.ascontiguousarray(xyz, np.float64)
        lib().ov2h_map_add_kp(self.h, 0, int(lmid), float(px[0]), float(px[1]), int(xyz is not None), None if x is None else _dp(x))

    def forget_landmark(self, lmid):
        lib().ov2h_map_forget_landmark(self.h, int(lmid))

    def stereo_matching(self, ctx, img_left, img_right):
        u8 = C.POINTER(C.c_uint8)
        a, b = np.ascontiguousarray(img_left, np.uint8), np.ascontiguousarray(img_right, np.uint8)
        return lib().ov2h_stereo_matching(self.h, ctx.h, 0, a.ctypes.data_as(u8), b.ctypes.data_as(u8), self.w, self.h_img)

    def klt_tracking(self, ctx, img_prev, img_cur):
        u8 = C.POINTER(C.c_uint8)
        a, b = np.ascontiguousarray(img_prev, np.uint8), np.ascontiguousarray(img_cur, np.uint8)
        req = C.c_int(0)
        st = lib().ov2h_klt_tracking(self.h, ctx.h, 0, a.ctypes.data_as(u8), b.ctypes.data_as(u8), self.w, self.h_img, C.byref(req))
        return st, bool(req.value)

    def keypoints(self, cap=65536):
        """dict lmid -> (px (2,), is3d, is_stereo, rpx (2,))"""
        fpp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        lm, px, rp = np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        i3, ist = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        n = lib().ov2h_get_keypoints(self.h, 0, cap, lm.ctypes.data_as(C.POINTER(C.c_int)), px.ctypes.data_as(fpp),
                                     i3.ctypes.data_as(u8), ist.ctypes.data_as(u8), rp.ctypes.data_as(fpp))
        assert 0 <= n <= cap
        return {int(lm[k]): (px[k].copy(), bool(i3[k]), bool(ist[k]), rp[k].copy()) for k in range(n)}

    # -- VisualFrontEnd::computePose on this frame (the P3P stage included) ---------------------------------------------
    def set_p3p(self, dop3p=True, nransac_iter=100, fransac_err=3.0, bdo_random=False, seed=0):
        """dop3p / nransac_iter / fransac_err / bdo_random of the YAML + the sampler's base seed; clears a pending P3P request"""
        lib().ov2h_set_p3p(self.h, int(bool(dop3p)), int(nransac_iter), float(fransac_err), int(bool(bdo_random)),
                           int(seed) & ((1 << 64) - 1))

    def compute_pose(self, ctx, Twc_init):
        """computePose from pose Twc_init; the P3P request is kept between calls. returns (status, p3p requested)"""
        req = C.c_int()
        st = lib().ov2h_compute_pose(self.h, ctx.h, 0, _dp(np.ascontiguousarray(Twc_init, np.float64)), C.byref(req))
        return st, bool(req.value)

    def p3p_stats(self):
        """what the P3P branch did in the last compute_pose: dict(ran, status, points, removed, reset)"""
        e = np.zeros(5)
        lib().ov2h_p3p_stats(self.h, _dp(e))
        return dict(ran=int(e[0]), status=int(e[1]), points=int(e[2]), removed=int(e[3]), reset=int(e[4]))

    def pose(self):
        out = np.zeros(7)
        assert lib().ov2h_get_pose(self.h, 0, _dp(out)) == 0
        return out

    def counters(self):
        """dict(nbkps, nb2dkps, nb3dkps, nb_stereo_kps, noccupcells) of the frame"""
        c = np.zeros(5, np.int32)
        assert lib().ov2h_frame_counters(self.h, 0, c.ctypes.data_as(C.POINTER(C.c_int))) == 0
        return dict(zip(("nbkps", "nb2dkps", "nb3dkps", "nb_stereo_kps", "noccupcells"), c.tolist()))

    def landmark_isobs(self, lmid):
        return lib().ov2h_landmark_isobs(self.h, int(lmid))

    def frl(self):
        F = np.zeros(9)
        lib().ov2h_get_frl(self.h, 0, _dp(F))
        return F.reshape(3, 3)

    def close(self):
        if getattr(self, "h", None):
            lib().ov2h_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
