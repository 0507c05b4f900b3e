// Flat device-resident map mirror + the set-up stage of Optimizer::localBA as linear scans.
//
// The reference keeps the map as hash maps of shared_ptr<Frame> / shared_ptr<MapPoint> (include/map_manager.hpp:41-129,
// include/frame.hpp mapkps_/map_covkfs_, include/map_point.hpp set_kfids_) and assembles every local BA by walking
// them (src/optimizer.cpp:43-430): ~4.4 ms for 40 keyframes / 3 k landmarks / 38 k residual blocks in the C++ mirror
// of that walk (ov2slam_amd/host), the same order as the solve itself.  Here the map is three SoA tables in HBM
// (keyframes, landmarks, observations; kfid and lmid index them directly; the tables grow on demand) and the set-up is a dozen scans of the
// observation table -- HBM-bound integer work: at 8 TB/s a million observations (40 B each) are a 5 us read, so no
// per-landmark adjacency needs to be maintained incrementally, the table itself is the adjacency.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ov2_cam.h"
#include "ov2_internal.h"
#include "ov2_se3.h"
#include "ov2_wave.h"
#include "tri_pair.h"

struct ov2_map {
    ov2_ctx *c;
    int max_kf, max_lm, max_obs, n_obs;
    int n_compactions;                                              // times the observation table was squeezed
    // tables
    double *kf_pose; unsigned char *kf_state;                       // [max_kf]
    double *lm_xyz; unsigned char *lm_state;                        // [max_lm]
    int *obs_kf, *obs_lm, *obs_scale; double *obs_uv, *obs_ruv; unsigned char *obs_flag;   // [max_obs]
    // set-up scratch
    int *hdr;                                                       // MH_N ints
    int *cov, *kf_role, *kf_idx;                                    // [max_kf]
    int *lm_nobs, *lm_sel, *lm_anchor, *lm_flag;                    // [max_lm]; lm_sel: 0 none, 1 local, 2 bad
    unsigned long long *lm_pack, *lm_pidx;                          // [max_lm] (flag | bad << 32) and its exclusive scan: (lm index | bad index << 32)
    unsigned char *lm_new;                                          // [max_lm] observed by the new keyframe
    int *obs_cnt, *obs_off;                                         // [max_obs]
    int *blk;                                                       // block sums of the scans
    unsigned char *zero_blk; size_t zero_bytes;                     // hdr | cov | kf_role | lm_nobs | lm_sel | lm_anchor | lm_new: one memset per set-up
    // outputs: device image + pinned host image of the flat problem
    unsigned char *out_dev, *out_host;
    size_t out_cap, out_host_cap;
    int *hdr_host;                                                  // pinned
    // the last set-up (the update stage reads its scratch arrays and its flat problem where they were left)
    int last_hdr[16];                                               // host copy of its header
    int last_newkf, last_inv, last_valid;
    int last_n_obs;                                                 // rows the last set-up saw (only they carry its obs_cnt / obs_off)
    int last_updated;                                               // its update stage has been enqueued: a second one is refused
    int last_kind;                                                  // 0: set-up of localBA, 1: of looseBA (each update stage takes its own kind only)
    int live_rows, live_known;                                      // live rows of the table as the last set-up counted them
    double last_K[4]; int have_K;                                   // left intrinsics (anchored inverse depth -> world point)
    // ov2_map_save_state / ov2_map_restore_state_batch
    double *snap_kf_pose, *snap_lm_xyz; unsigned char *snap_kf_state, *snap_lm_state, *snap_obs_flag;
    int snap_kf, snap_lm, snap_obs;
    int snap_floor;                                                 // rows a squeeze kept for the saved state: no new squeeze below 2x
    // ov2_map_triangulate_temporal_batch: scratch and output lists of its own (the arrays of the last set-up stay as they are)
    unsigned char *tt_zero; size_t tt_zero_bytes;                   // hdr (MH_N ints) | tt_nobs | tt_old | tt_nrow: one clear per call
    int *tt_nobs, *tt_old, *tt_nrow;                                // [max_lm] observers, ANCH_TOP - oldest observer, row of the new keyframe + 1
    int *tt_int;                                                    // [3 max_lm] row of the oldest observer | good_lmid | removed_lmid
    double *tt_dbl;                                                 // [4 max_lm] good_wpt (x3) | good_invdepth
    // ov2_map_triangulate_stereo_batch / ov2_map_set_obs_stereo_batch_dev: scratch and output lists of their own as well
    unsigned char *ts_zero; size_t ts_zero_bytes;                   // hdr (MH_N ints) | ts_mark: the stage clears the header, the intake both
    int *ts_mark;                                                   // [max_lm] entry of the intake's list + 1 (the last one that names the landmark)
    int *ts_int;                                                    // [2 max_lm] good_lmid | demoted_lmid
    double *ts_dbl;                                                 // [4 max_lm] good_wpt (x3) | good_invdepth
    unsigned char *ts_why;                                          // [max_lm] demoted_why
    // host copy of kf_state (which keyframes live), so that a call can refuse a dead keyframe without a synchronisation
    unsigned char *kf_alive_h, *snap_kf_alive_h;
    // ov2_map_filter_keyframes_batch: scratch of its own as well
    unsigned char *fl_zero; size_t fl_zero_bytes;                   // hdr (MH_N ints) | fl_nobs | fl_cov | fl_n3d | fl_cnt | fl_fill | fl_new: one clear per call
    int *fl_nobs;                                                   // [max_lm] observers; the walk decrements them
    int *fl_cov, *fl_n3d, *fl_cnt, *fl_fill;                        // [max_kf] covisibility with newkf, 3D rows, live rows, rows scattered so far
    unsigned char *fl_new;                                          // [max_lm] observed by the new keyframe
    int *fl_start;                                                  // [max_kf] exclusive scan of fl_cnt: where the keyframe's rows start in fl_rows
    int *fl_rows;                                                   // [max_obs] live rows grouped by keyframe
    int *fl_unset;                                                  // [max_lm] landmarks whose OV2_LM_3D the walk cleared
    int *fl_removed_h; int fl_removed_cap;                          // pinned: the removed keyframes of the last call
    // ov2_map_merge_points_batch: scratch of its own again
    unsigned char *mg_zero; size_t mg_zero_bytes;                   // hdr (MH_N ints) | mg_cnt | mg_fill | mg_next | mg_stamp | mg_mark: one clear per call
    int *mg_cnt, *mg_fill, *mg_next;                                // [max_lm] live rows of a named landmark, rows scattered so far, adopted segment + 1
    int *mg_stamp;                                                  // [max_kf] pair index + 1 of the last pair whose `new` the keyframe observes
    unsigned char *mg_mark;                                         // [max_lm] named by a pair of the call
    int *mg_start;                                                  // [max_lm] exclusive scan of mg_cnt: where the landmark's rows start in mg_rows
    int *mg_rows;                                                   // [max_obs] live rows of the named landmarks, grouped by landmark
    // ov2_map_enable_match_columns: raw pixel, descriptor and "has a descriptor" per observation row (all null without it)
    float *obs_px; unsigned char *obs_desc, *obs_hasdesc;           // [max_obs] x 2 floats, x 32 bytes, x 1
    int *mg_srow;                                                   // [max_kf] the row behind mg_stamp: `new`'s row of the keyframe
    int *gt_seen_h; int gt_gen;                                     // host, [max_lm]: the call that last listed the landmark (duplicates are refused)
    // ov2_map_structure_ba_batch: the solver's state, O(listed entries), allocated with the first call (null before it)
    unsigned char *sb_ws; int sb_cap;                               // sb_cap entries: SP_N doubles per point | the entered ids
    // ov2_map_enable_local_sets: Frame::set_local_mapids_ per keyframe, ascending lmid, in one id pool (all null / 0 without it)
    int ls_on;
    int *ls_start, *ls_count;                                       // [max_kf] where the keyframe's set starts in the pool, its size (0: none)
    int *ls_start_h, *ls_count_h;                                   // host copies of both
    int *ls_pool; int ls_pool_cap, ls_pool_used, ls_live;           // the pool: entries allocated / appended so far / of the sets that count
    int ls_squeezes;                                                // times the pool was squeezed
    // ov2_map_local_ids_batch: scratch of its own
    unsigned char *ls_zero; size_t ls_zero_bytes;                   // hdr (MH_N ints) | ls_cov | ls_mark | ls_obs: one clear per call
    int *ls_cov;                                                    // [max_kf] covisibility with the new keyframe
    int *ls_mark;                                                   // [max_lm] 1: the landmark is in the set being built
    unsigned char *ls_obs;                                          // [max_lm] observed by the new keyframe
    int *ls_pos;                                                    // [max_lm] exclusive scan of ls_mark: the landmark's place in the set
    int *ls_out_h; int ls_out_cap;                                  // pinned: cov_kfid | cov_score | lmid of the last call
};

namespace {

enum { MH_NBKPS = 0, MH_NB3D, MH_ABORT, MH_NMAXKF, MH_NPOSE, MH_NRES, MH_NLM, MH_NBAD, MH_NLIVE,   // NLM|NBAD: one 64-bit scan total
       MH_NEED16,                       // bytes / 16 the flat problem needs (written with the gathered header)
       MH_OVER,                         // ... and 1 when that exceeds the map's output block: nothing was emitted, the host grows it and re-runs
       MH_NRM_LM, MH_NRM_OBS, MH_NST_OFF,   // update stage: landmarks removed, observations removed, stereo observations demoted
       MH_N = 16 };
// header of the keyframe filter (its own block, cleared per call): what ov2_map_filter reports, and the scan total of the rows
enum { FH_CANDIDATES = 0, FH_REMOVED, FH_FEW3D, FH_UNSET3D, FH_ROWS };
// header of the map-point merge (its own block as well): the five counts of ov2_map_merge, and the scan total of the rows
enum { GH_PAIRS = 0, GH_MERGED, GH_SKIPPED, GH_MOVED, GH_CONFLICT, GH_ROWS };
// header of the local-map selection (its own block too): what ov2_map_local_ids reports.  LH_OLDMAX is the smallest covisible
// kfid as ANCH_TOP - kfid under atomicMax (0 = none), LH_NLOCAL the scan total of the marks
enum { LH_NCOV = 0, LH_OLDMAX, LH_NFRESH, LH_NLOCAL, LH_SWAPPED, LH_EXTENDED, LH_OLDEST };
#define ANCH_TOP 0x40000000   // anchor keyframe stored as ANCH_TOP - kfid under atomicMax: 0 = none, so the array lives in the zeroed block
enum { OBS_ALIVE = 1, OBS_STEREO = 2 };
enum { MAP_COMPACT_MIN_ROWS = 4096 };   // below this the scans cost nothing worth a reallocation

struct map_view {
    int max_kf, max_lm, n_obs;
    const double *kf_pose; const unsigned char *kf_state;
    const double *lm_xyz; const unsigned char *lm_state;
    const int *obs_kf, *obs_lm, *obs_scale; const double *obs_uv, *obs_ruv; const unsigned char *obs_flag;
    const float2 *obs_px; const uint4 *obs_desc; const unsigned char *obs_hasdesc;   // match columns, null without them
};

// an observation counts when it, its keyframe and its landmark are alive (MapPoint::set_kfids_ / Frame::mapkps_ agree)
__device__ __forceinline__ bool obs_live(const map_view &M, int i, int &kf, int &lm)
{
    if (!(M.obs_flag[i] & OBS_ALIVE)) return false;
    kf = M.obs_kf[i]; lm = M.obs_lm[i];
    return M.kf_state[kf] && (M.lm_state[lm] & OV2_LM_ALIVE);
}

// ---- hooks ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_set_lm_kernel(int n, const int *__restrict__ lmid, const double *__restrict__ xyz,
                                                         const unsigned char *__restrict__ state, double *__restrict__ lm_xyz,
                                                         unsigned char *__restrict__ lm_state)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = lmid[i];
    lm_state[l] = state[i];
    if (xyz) { lm_xyz[3 * l] = xyz[3 * i]; lm_xyz[3 * l + 1] = xyz[3 * i + 1]; lm_xyz[3 * l + 2] = xyz[3 * i + 2]; }
}

__global__ __launch_bounds__(256) void map_set_pose_kernel(int n, const int *__restrict__ kfid, const double *__restrict__ T,
                                                           double *__restrict__ kf_pose)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 7) return;
    kf_pose[7 * kfid[i / 7] + i % 7] = T[i];
}

// (kfid, lmid) pairs are few per call: every observation checks the list (list in LDS by chunks of 256)
// mode 0: kill the observation; mode 1: set / clear the stereo flag (+ runpx)
__global__ __launch_bounds__(256) void map_edit_obs_kernel(int n_obs, const int *__restrict__ obs_kf, const int *__restrict__ obs_lm,
                                                           unsigned char *__restrict__ obs_flag, double *__restrict__ obs_ruv,
                                                           int n, const int *__restrict__ kfid, const int *__restrict__ lmid,
                                                           int mode, const unsigned char *__restrict__ st,
                                                           const double *__restrict__ ruv)
{
    __shared__ int sk[256], sl[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_obs && (obs_flag[i] & OBS_ALIVE);
    const int k = live ? obs_kf[i] : -1, l = live ? obs_lm[i] : -1;
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) { sk[threadIdx.x] = kfid[base + threadIdx.x]; sl[threadIdx.x] = lmid[base + threadIdx.x]; }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; ++j)
            if (sl[j] == l && (sk[j] == k || sk[j] < 0)) {   // kfid < 0: every keyframe (removeMapPoint)
                if (mode == 0) obs_flag[i] = 0;
                else {
                    if (st[base + j]) {
                        obs_flag[i] |= OBS_STEREO;
                        obs_ruv[2 * i] = ruv[2 * (base + j)]; obs_ruv[2 * i + 1] = ruv[2 * (base + j) + 1];
                    } else obs_flag[i] &= ~OBS_STEREO;
                }
            }
    }
}

// MapPoint::addDesc(kfid, desc) for keyframes that observe the point: the same search, the live row (kfid, lmid) takes the
// pixel (where given), the descriptor and its flag
__global__ __launch_bounds__(256) void map_set_desc_kernel(int n_obs, const int *__restrict__ obs_kf, const int *__restrict__ obs_lm,
                                                           const unsigned char *__restrict__ obs_flag, float2 *__restrict__ obs_px,
                                                           uint4 *__restrict__ obs_desc, unsigned char *__restrict__ obs_hasdesc, int n,
                                                           const int *__restrict__ kfid, const int *__restrict__ lmid,
                                                           const float2 *__restrict__ px, const uint4 *__restrict__ desc,
                                                           const unsigned char *__restrict__ has)
{
    __shared__ int sk[256], sl[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_obs && (obs_flag[i] & OBS_ALIVE);
    const int k = live ? obs_kf[i] : -1, l = live ? obs_lm[i] : -1;
    for (int base = 0; base < n; base += 256) {
        const int m = min(256, n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) { sk[threadIdx.x] = kfid[base + threadIdx.x]; sl[threadIdx.x] = lmid[base + threadIdx.x]; }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; ++j)
            if (sl[j] == l && sk[j] == k) {
                if (px) obs_px[i] = px[base + j];
                obs_hasdesc[i] = has[base + j] ? 1 : 0;
                if (has[base + j]) { obs_desc[2 * (size_t)i] = desc[2 * (size_t)(base + j)]; obs_desc[2 * (size_t)i + 1] = desc[2 * (size_t)(base + j) + 1]; }
            }
    }
}

// ---- batched set-up / update ---------------------------------------------------------------------------
// Every kernel below serves B maps in one launch: the map is blockIdx.y, its tables and scratch arrays come from a
// device table of map_job records (one H2D copy per call).  Sizes that a later kernel needs (poses, landmarks, residual
// blocks of the flat problem) are read from the map's device-side header, never from the host: the whole chain is
// enqueued without a synchronisation.
struct map_job {
    map_view M;
    int newkf, cur_kfid;
    int last_n_obs;                              // update stage: rows of the set-up (rows appended since have no obs_cnt / obs_off)
    int *hdr, *cov, *kf_role, *kf_idx, *lm_nobs, *lm_sel, *lm_anchor, *lm_flag;
    unsigned long long *lm_pack, *lm_pidx;
    unsigned char *lm_new;
    int *obs_cnt, *obs_off;
    void *blk;                                   // block sums of the scans
    unsigned char *zero_blk; unsigned zero_vec16; // the zeroed block, in 16-byte units
    unsigned char *out; unsigned long long out_cap;
    int *hdr_out;                                // this map's slot of the gathered headers (one D2H for all maps)
    // writable twins of the tables (update stage, restore)
    double *kf_pose_w, *lm_xyz_w; unsigned char *kf_state_w, *lm_state_w, *obs_flag_w;
    const unsigned char *outlier;                // update stage: per residual block flags of the solve (may be null)
    double K[4];                                 // left intrinsics (update stage, inverse depth)
    const double *snap_kf_pose, *snap_lm_xyz; const unsigned char *snap_kf_state, *snap_lm_state, *snap_obs_flag;
    int snap_kf, snap_lm, snap_obs;
    // temporal triangulation (hdr / zero_blk point at the stage's own block in its job records)
    int *tt_nobs, *tt_old, *tt_nrow, *tt_arow, *tt_good_lmid, *tt_rm_lmid;
    double *tt_good_wpt, *tt_good_inv;
    // stereo triangulation and the intake of the matcher's verdicts (hdr / zero_blk point at the stage's own block in its job records)
    double st_Kr[4], st_Tlr[7]; int st_rect;     // the rig: K holds the left intrinsics, these the right ones, Tlr and bdo_stereo_rect_
    int *ts_mark, *ts_good_lmid, *ts_dem_lmid;
    double *ts_good_wpt, *ts_good_inv;
    unsigned char *ts_why;
    double *obs_ruv_w;                           // writable twin of obs_ruv (the intake)
    int si_n;                                    // the intake's list of this map: entries, ids, status bytes, raw right pixels
    const int *si_lmid; const unsigned char *si_status; const float *si_rxy;
    ov2_cam_model si_cam;                        // the right camera's lens model (model 0: identity)
    // keyframe filter (hdr / zero_blk point at the stage's own block in its job records; hdr_out is followed by the removed list)
    int fl_active;                               // 0: gated map (ratio >= 1 or newkf < 20), zero header and no work
    int *fl_nobs, *fl_cov, *fl_n3d, *fl_cnt, *fl_fill, *fl_start, *fl_rows, *fl_unset;
    unsigned char *fl_new;
    // pose-graph update (hdr / zero_blk point at the temporal stage's block; the anchor scan lands in tt_old)
    int pg_n;                                    // free keyframes of the graph, 0: nothing to do for this map
    const int *pg_kfid; const double *pg_Twc;    // their ids (ascending, last = newkf) and optimised poses, in the staging block
    double *pg_tmp;                              // 14 doubles behind hdr_out: inverse(old(newkf)) | T_corr
    const unsigned char *pg_skip;                // null (host form), or one byte in device memory: non-zero = leave this map alone
    // local pose graph, assembly and gate (hdr / zero_blk as for the update): the lp_n poses of the chain (0: no chain) are
    // the keyframes lp_kfid (the loop keyframe, then ascending up to newkf); pg_kfid / pg_Twc / pg_skip above name the same
    // block past its first pose
    int lp_n, lp_stereo;
    const int *lp_kfid; const double *lp_newTwc; // the loop pose the graph is built for
    double *lp_pose, *lp_Tij;                    // the problem block: lp_n poses | lp_n edges, the closing edge last
    unsigned char *lp_skip; int *lp_verdict, *lp_npairs;   // what the gate writes (lp_npairs may be null)
    // merge of map points (hdr / zero_blk point at the stage's own block in its job records)
    int mg_seg;                                  // pairs in this map's segment of the lists, 0: nothing to do for this map
    const int *mg_prev, *mg_new;                 // the segment: prevlmid / newlmid per pair, in list order
    const unsigned char *mg_cur;                 // per pair: the current frame held prevlmid (may be null)
    const int *mg_n_dev;                         // null, or how many pairs of the segment count (device memory)
    unsigned char *mg_status;                    // per pair: OV2_MERGE_* (may be null)
    int *mg_cnt, *mg_fill, *mg_next, *mg_stamp, *mg_start, *mg_rows;
    unsigned char *mg_mark;
    int *obs_lm_w;                               // writable twin of obs_lm (the walk relabels rows)
    // match columns: what the walk's conflict rule edits (null without the columns)
    uint4 *obs_desc_w; unsigned char *obs_hasdesc_w; int *mg_srow;
    // match gather (hdr / zero_blk point at the merge stage's block; mg_seg = entries of this map, 0: nothing to do)
    int gt_on;                                   // 1: the mark kernel reads the two id lists below instead of the pairs
    int gt_nkp, gt_ncand, gt_kp0, gt_cand0, gt_kf0;   // this map's keypoints / candidates and where they and its poses start in the flat arrays
    const int *gt_kp_lmid, *gt_cand_lmid;        // this map's segments of the id lists
    // flat scans of the gather (records behind the B maps): the array is scanned in place, the total lands behind it
    int *gt_scan; int gt_scan_n;
    // structure-only BA (hdr / zero_blk point at the merge stage's block; mg_seg = entries of this map's segment, mg_new = the
    // segment of the id list, mg_n_dev = how many of them are looked at; hdr_out takes the map's ov2_map_sba record)
    int sb_on;                                   // 1: the mark kernel reads the id list instead of the pairs
    const unsigned char *sb_status;              // null, or per entry: it counts iff its byte is OV2_MERGE_DONE
    const double *sb_cam;                        // this map's ov2_map_sba_cam
    double *sb_pt; int *sb_lm;                   // the solver's block: SP_N doubles per entered point | their ids in list order
    // looseBA: set-up (lb_lo = first keyframe of the range, newkf = the loop keyframe) and update (lb_on = 0: no-op map;
    // lb_cnt / lb_tmp: LB_N counters and inverse(old(newkf)) | opt | T_corr behind the map's gathered header)
    int lb_lo, lb_on;
    int *lb_cnt; double *lb_tmp;
    // local-map selection (hdr / zero_blk point at the stage's own block in its job records; hdr_out is followed by
    // ls_kcap covisible kfids | ls_kcap scores | ls_room lmids)
    int ls_on;                                   // 1 in the records of ov2_map_local_ids_batch: the scan reads ls_mark
    int ls_extend, ls_nmax;                      // the extension of Mapper::matchingToLocalMap is asked for / its size gate
    int ls_kcap, ls_room;                        // entries of the two covisibility lists / of the id list, in the gathered copy and in the pool
    int ls_pool_off;                             // where the new set starts in the pool (ls_pool_off + ls_room <= its capacity)
    int *ls_cov, *ls_mark, *ls_pos, *ls_pool, *ls_start, *ls_count;
    unsigned char *ls_obs;
};

// the flat arrays of a gather call (ov2_match_batch_input as the kernels write it) and their row capacity
struct gather_out {
    double *Twc; float2 *kp_px; int *kp_desc_ptr, *kp_kf_ptr, *kp_kfids; float2 *kp_kf_px; uint4 *kp_descs;
    double *cand_wpt; int *cand_desc_ptr, *cand_kf_ptr, *cand_kfids; uint4 *cand_descs; double *kf_Twc;
    int cap_rows;                                // entries kp_kfids / cand_kfids (and the descriptor arrays) can hold
};

// the flat problem of one map inside its output block: the same carve on the device (emitters, update stage) and on the
// host (pointer translation), from the four counts of the header
enum { FO_POSE_KFID = 0, FO_POSE_CONST, FO_POSE, FO_LM_LMID, FO_LM, FO_LM_ANCH, FO_LM_AUV, FO_RES_TYPE, FO_RES_POSE, FO_RES_LM,
       FO_RES_UV, FO_RES_SIGMA, FO_BAD, FO_HOST_END,   // [0, FO_HOST_END): what the host form copies to pinned memory
       FO_RES_OUT = FO_HOST_END, FO_RM_LM, FO_RM_OBS, FO_ST_OFF, FO_N };

__host__ __device__ inline size_t flat_layout(size_t P, size_t NL, size_t R, size_t NB, int e, size_t *off)
{
    size_t o = 0;
#define CARVE(k, bytes) do { off[k] = o; o = (o + (size_t)(bytes) + 15) & ~(size_t)15; } while (0)
    CARVE(FO_POSE_KFID, P * 4); CARVE(FO_POSE_CONST, P); CARVE(FO_POSE, P * 56); CARVE(FO_LM_LMID, NL * 4); CARVE(FO_LM, NL * 8 * e);
    CARVE(FO_LM_ANCH, NL * 4); CARVE(FO_LM_AUV, NL * 16); CARVE(FO_RES_TYPE, R); CARVE(FO_RES_POSE, R * 4); CARVE(FO_RES_LM, R * 4);
    CARVE(FO_RES_UV, R * 16); CARVE(FO_RES_SIGMA, R * 8); CARVE(FO_BAD, NB * 4);
    // device only: the solver's per-block outlier flags, and what the update stage reports back
    CARVE(FO_RES_OUT, R); CARVE(FO_RM_LM, (NL + NB) * 4); CARVE(FO_RM_OBS, R * 8); CARVE(FO_ST_OFF, R * 8);
#undef CARVE
    return o;
}

struct flat_out {
    int *pose_kfid; unsigned char *pose_const; double *pose;
    int *lm_lmid; double *lm; int *lm_anchor_pose; double *lm_anchor_uv;
    unsigned char *res_type; int *res_pose, *res_lm; double *res_uv, *res_sigma;
    int *bad_lmid;
    unsigned char *res_out; int *rm_lm; int2 *rm_obs, *st_off;
};

__host__ __device__ inline flat_out flat_ptrs(unsigned char *D, const size_t *off)
{
    flat_out O;
    O.pose_kfid = (int *)(D + off[FO_POSE_KFID]); O.pose_const = D + off[FO_POSE_CONST]; O.pose = (double *)(D + off[FO_POSE]);
    O.lm_lmid = (int *)(D + off[FO_LM_LMID]); O.lm = (double *)(D + off[FO_LM]); O.lm_anchor_pose = (int *)(D + off[FO_LM_ANCH]);
    O.lm_anchor_uv = (double *)(D + off[FO_LM_AUV]); O.res_type = D + off[FO_RES_TYPE]; O.res_pose = (int *)(D + off[FO_RES_POSE]);
    O.res_lm = (int *)(D + off[FO_RES_LM]); O.res_uv = (double *)(D + off[FO_RES_UV]); O.res_sigma = (double *)(D + off[FO_RES_SIGMA]);
    O.bad_lmid = (int *)(D + off[FO_BAD]); O.res_out = D + off[FO_RES_OUT]; O.rm_lm = (int *)(D + off[FO_RM_LM]);
    O.rm_obs = (int2 *)(D + off[FO_RM_OBS]); O.st_off = (int2 *)(D + off[FO_ST_OFF]);
    return O;
}

__device__ __forceinline__ flat_out flat_of(const map_job &j, int inv, bool *fits = nullptr)
{
    const int *H = j.hdr;
    size_t off[FO_N];
    const size_t need = flat_layout((size_t)H[MH_NPOSE], (size_t)H[MH_NLM], (size_t)H[MH_NRES], (size_t)H[MH_NBAD], inv ? 1 : 3, off);
    if (fits) *fits = need <= j.out_cap;
    return flat_ptrs(j.out, off);
}

__global__ __launch_bounds__(256) void mb_zero_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    uint4 *z = reinterpret_cast<uint4 *>(j.zero_blk);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < j.zero_vec16; i += gridDim.x * 256) z[i] = zero;
}

// ---- set-up scans -----------------------------------------------------------------------------------
// observers per landmark, landmarks of the new keyframe, its keypoint counts (Frame::nbkps_, nb3dkps_)
__global__ __launch_bounds__(256) void ms_count_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    const bool live = i < M.n_obs && obs_live(M, i, kf, lm);
    // live rows of the table (one atomic per wave): the host compacts the table when most rows are dead
    const unsigned long long bal = __ballot(live);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&j.hdr[MH_NLIVE], __popcll(bal));
    if (!live) return;
    atomicAdd(&j.lm_nobs[lm], 1);
    if (kf == j.newkf) {
        j.lm_new[lm] = 1;
        atomicAdd(&j.hdr[MH_NBKPS], 1);
        if (M.lm_state[lm] & OV2_LM_KP3D) atomicAdd(&j.hdr[MH_NB3D], 1);
    }
}

// ---- compaction of the observation table ------------------------------------------------------------
// Observations are appended and killed in place (tombstones), so a long sequence leaves mostly dead rows behind
// (the reference erases them from its hash maps: src/map_manager.cpp:885-1019).  Dead rows (flag cleared, or keyframe /
// landmark gone -- neither id is ever reused) are squeezed out by a stable scatter: the row order, and so every set-up
// result, stays what it was.  With a saved state (ov2_map_save_state), a row that is live in EITHER state is kept and the
// saved observation flags are squeezed by the same scatter, so that ov2_map_restore_state_batch still rewinds the map.
struct snap_view { const unsigned char *kf_state, *lm_state, *obs_flag; };   // obs_flag == nullptr: no saved state to keep

__global__ __launch_bounds__(256) void mc_mark_kernel(map_view M, snap_view S, int *__restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M.n_obs) return;
    int kf, lm;
    bool k = obs_live(M, i, kf, lm);
    if (!k && S.obs_flag) {
        kf = M.obs_kf[i]; lm = M.obs_lm[i];
        k = (S.obs_flag[i] & OBS_ALIVE) && S.kf_state[kf] && (S.lm_state[lm] & OV2_LM_ALIVE);
    }
    keep[i] = k ? 1 : 0;
}

struct obs_cols { int *kf, *lm, *scale; double *uv, *ruv; unsigned char *flag, *snap_flag; float *px; unsigned char *desc, *hasdesc; };

__global__ __launch_bounds__(256) void mc_scatter_kernel(map_view M, const unsigned char *__restrict__ snap_flag, const int *__restrict__ keep,
                                                         const int *__restrict__ pos, obs_cols O)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M.n_obs || !keep[i]) return;
    const int j = pos[i];
    O.kf[j] = M.obs_kf[i]; O.lm[j] = M.obs_lm[i]; O.scale[j] = M.obs_scale[i]; O.flag[j] = M.obs_flag[i];
    if (snap_flag) O.snap_flag[j] = snap_flag[i];
    reinterpret_cast<double2 *>(O.uv)[j] = reinterpret_cast<const double2 *>(M.obs_uv)[i];
    reinterpret_cast<double2 *>(O.ruv)[j] = reinterpret_cast<const double2 *>(M.obs_ruv)[i];
    if (M.obs_hasdesc) {   // the match columns travel with the row
        reinterpret_cast<float2 *>(O.px)[j] = M.obs_px[i];
        reinterpret_cast<uint4 *>(O.desc)[2 * (size_t)j] = M.obs_desc[2 * (size_t)i];
        reinterpret_cast<uint4 *>(O.desc)[2 * (size_t)j + 1] = M.obs_desc[2 * (size_t)i + 1];
        O.hasdesc[j] = M.obs_hasdesc[i];
    }
}

// MapManager::updateFrameCovisibility (src/map_manager.cpp:117-193): co-observed landmarks per other keyframe
__global__ __launch_bounds__(256) void ms_cov_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i >= M.n_obs || !obs_live(M, i, kf, lm)) return;
    if (kf != j.newkf && j.lm_new[lm]) atomicAdd(&j.cov[kf], 1);
}

// src/optimizer.cpp:61-63,128-190: one wave walks the covisible keyframes newest -> oldest, 64 per step.
// kf_role: 0 = not in the problem, 1 = optimised, 2 = constant
__global__ __launch_bounds__(64) void ms_select_kernel(const map_job *__restrict__ J, int nmin_cov)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    int *hdr = j.hdr;
    const int newkf = j.newkf;
    const int lane = threadIdx.x;
    const int nb3d = hdr[MH_NB3D], nbkps = hdr[MH_NBKPS];
    if (nb3d < nmin_cov) { if (lane == 0) hdr[MH_ABORT] = 1; return; }
    bool all_cst = false;
    int nmax = -1;
    for (int hi = M.max_kf - 1; hi >= 0; hi -= 64) {
        const int kf = hi - lane;
        bool in = false, good = false;
        if (kf >= 0 && M.kf_state[kf]) {
            int score = (kf == newkf) ? nb3d : j.cov[kf];
            in = (kf == newkf) || score > 0;
            if (kf > newkf) score = nbkps;
            good = score >= nmin_cov && kf > 0;
        }
        const unsigned long long min_ = __ballot(in), bad_ = __ballot(in && !good);
        if (nmax < 0 && min_) nmax = hi - (__ffsll((long long)min_) - 1);   // lane 0 holds the largest kfid of the step
        // lanes after (older than) the first failing one are constant too
        bool cst = all_cst;
        if (bad_) {
            const int first_bad = __ffsll((long long)bad_) - 1;
            if (lane >= first_bad) cst = true;
            all_cst = true;
        }
        if (in) j.kf_role[kf] = cst ? 2 : 1;
    }
    if (lane == 0) hdr[MH_NMAXKF] = nmax;
}

// landmarks of the optimised keyframes' 3D keypoints (:176-180) and MapPoint::isBad (src/map_point.cpp:215-234)
__global__ __launch_bounds__(256) void ms_local_lm_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (j.hdr[MH_ABORT] || i >= M.n_obs || !obs_live(M, i, kf, lm)) return;
    const int st = M.lm_state[lm];
    if (j.kf_role[kf] != 1 || !(st & OV2_LM_KP3D)) return;
    const int nobs = j.lm_nobs[lm];
    const bool isobs = st & OV2_LM_OBS;
    const bool bad = (nobs < 2 && !isobs && (st & OV2_LM_3D)) || (nobs == 0 && !isobs);
    j.lm_sel[lm] = bad ? 2 : 1;
}

// observers of the local landmarks: outside keyframes become constant poses (:229-246), the first observer anchors
// the landmark (:251-287).  (The update stage recounts observers and oldest observers from the table as it is then.)
__global__ __launch_bounds__(256) void ms_observers_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (j.hdr[MH_ABORT] || i >= M.n_obs || !obs_live(M, i, kf, lm)) return;
    if (j.lm_sel[lm] != 1 || kf > j.hdr[MH_NMAXKF]) return;
    if (j.kf_role[kf] == 0) j.kf_role[kf] = 2;     // every writer stores the same value
    atomicMax(&j.lm_anchor[lm], ANCH_TOP - kf);     // the smallest kfid wins
}

// gauge (:394-407) + dense pose numbering in ascending kfid.  One workgroup per map.
__global__ __launch_bounds__(1024) void ms_poses_kernel(const map_job *__restrict__ J, int nmin_cst)
{
    const map_job &j = J[blockIdx.y];
    const int max_kf = j.M.max_kf;
    int *kf_role = j.kf_role, *kf_idx = j.kf_idx, *hdr = j.hdr;
    __shared__ int wsum[16], carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (hdr[MH_ABORT]) return;
    // constants so far
    int ncst = 0;
    for (int k = tid; k < max_kf; k += 1024) ncst += kf_role[k] == 2;
    for (int o = 32; o; o >>= 1) ncst += __shfl_xor(ncst, o);
    if (lane == 0) wsum[wv] = ncst;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < 16; ++w) t += wsum[w];
        // not enough constants: the smallest optimised kfids are fixed (serial: at most nmin_cst <= 2 hits)
        for (int k = 0; k < max_kf && t < nmin_cst; ++k)
            if (kf_role[k] == 1) { kf_role[k] = 2; ++t; }
        carry_s = 0;
    }
    __syncthreads();
    for (int base = 0; base < max_kf; base += 1024) {
        const int k = base + tid;
        const int f = (k < max_kf && kf_role[k] != 0) ? 1 : 0;
        int x = f;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int off = carry_s;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (k < max_kf) kf_idx[k] = f ? off + x - 1 : -1;
        __syncthreads();
        if (tid == 1023) carry_s = off + x;
        __syncthreads();
    }
    if (tid == 0) hdr[MH_NPOSE] = carry_s;
}

// flags of the landmark numbering: local and (with inverse depth) anchored; bad ones go to their own list.  Both flags
// ride one 64-bit word so that one scan numbers both lists.
__global__ __launch_bounds__(256) void ms_lm_flags_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= j.M.max_lm) return;
    const int s = j.lm_sel[l];
    const int f = (s == 1 && (!inv || j.lm_anchor[l] != 0)) ? 1 : 0;
    j.lm_flag[l] = f;
    j.lm_pack[l] = (unsigned long long)f | ((unsigned long long)(s == 2) << 32);
}

// residual blocks per observation (:251-391): anchor observation 1 if stereo (right-anchor block) else 0; any other
// observation 2 if stereo (left + right) else 1
__global__ __launch_bounds__(256) void ms_res_count_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M.n_obs) return;
    int kf, lm, c = 0;
    if (!j.hdr[MH_ABORT] && obs_live(M, i, kf, lm) && j.lm_flag[lm] && kf <= j.hdr[MH_NMAXKF]) {
        const bool stereo = M.obs_flag[i] & OBS_STEREO;
        if (inv && j.lm_anchor[lm] == ANCH_TOP - kf) c = stereo ? 1 : 0;
        else c = stereo ? 2 : 1;
    }
    j.obs_cnt[i] = c;
}

// ---- exclusive scan of an array (int, or two counters packed in 64 bits) in three launches:
// block sums -> their scan -> block offsets.  `which` selects the array of the map: SC_LM the landmark flags (64-bit,
// total -> NLM | NBAD), SC_RES the residual counts (total -> NRES), SC_LIVE the keep flags of a compaction (total -> NLIVE),
// SC_KF the live rows per keyframe of the keyframe filter (total -> FH_ROWS of its header)
// SC_MG the live rows per named landmark of the map-point merge (total -> GH_ROWS of its header)
// SC_GT a flat count array of the match gather, in place (total -> the entry behind the array: the n + 1 prefix offsets)
// SC_LS the landmark marks of the local-map selection (total -> LH_NLOCAL of its header)
enum { SC_LM = 0, SC_RES, SC_LIVE, SC_KF, SC_MG, SC_GT, SC_LS };

template <typename T>
__device__ __forceinline__ T shfl_up_t(T v, int o)
{
    if constexpr (sizeof(T) == 8) {
        const unsigned lo = (unsigned)__shfl_up((int)(v & 0xffffffffull), o), hi = (unsigned)__shfl_up((int)(v >> 32), o);
        return ((T)hi << 32) | lo;
    } else {
        return __shfl_up(v, o);
    }
}

template <typename T>
__device__ __forceinline__ void scan_args(const map_job &j, int which, const T *&in, T *&out, T *&blk, T *&total, int &n)
{
    blk = reinterpret_cast<T *>(j.blk);
    if (which == SC_LM) {
        in = reinterpret_cast<const T *>(j.lm_pack); out = reinterpret_cast<T *>(j.lm_pidx); n = j.M.max_lm;
        total = reinterpret_cast<T *>(j.hdr + MH_NLM);
    } else if (which == SC_KF) {
        in = reinterpret_cast<const T *>(j.fl_cnt); out = reinterpret_cast<T *>(j.fl_start); n = j.fl_active ? j.M.max_kf : 0;
        total = reinterpret_cast<T *>(j.hdr + FH_ROWS);
    } else if (which == SC_MG) {
        in = reinterpret_cast<const T *>(j.mg_cnt); out = reinterpret_cast<T *>(j.mg_start); n = j.mg_seg ? j.M.max_lm : 0;
        total = reinterpret_cast<T *>(j.hdr + GH_ROWS);
    } else if (which == SC_GT) {
        in = reinterpret_cast<const T *>(j.gt_scan); out = reinterpret_cast<T *>(j.gt_scan); n = j.gt_scan_n;
        total = reinterpret_cast<T *>(j.gt_scan + j.gt_scan_n);
    } else if (which == SC_LS) {
        in = reinterpret_cast<const T *>(j.ls_mark); out = reinterpret_cast<T *>(j.ls_pos); n = j.ls_on ? j.M.max_lm : 0;
        total = reinterpret_cast<T *>(j.hdr + LH_NLOCAL);
    } else {
        in = reinterpret_cast<const T *>(j.obs_cnt); out = reinterpret_cast<T *>(j.obs_off); n = j.M.n_obs;
        total = reinterpret_cast<T *>(j.hdr + (which == SC_RES ? MH_NRES : MH_NLIVE));
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void scan_block_kernel(const map_job *__restrict__ J, int which)
{
    const T *in; T *out, *blk, *total; int n;
    scan_args<T>(J[blockIdx.y], which, in, out, blk, total, n);
    if ((int)blockIdx.x * 1024 >= n) return;
    __shared__ T wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.x * 1024 + tid;
    const T v = i < n ? in[i] : (T)0;
    T x = v;
    for (int o = 1; o < 64; o <<= 1) { const T y = shfl_up_t(x, o); if (lane >= o) x += y; }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    T off = 0;
    for (int w = 0; w < wv; ++w) off += wsum[w];
    if (i < n) out[i] = off + x - v;
    if (tid == 1023) blk[blockIdx.x] = off + x;
}

template <typename T>
__global__ __launch_bounds__(1024) void scan_top_kernel(const map_job *__restrict__ J, int which)
{
    const T *in; T *out, *blk, *total; int n;
    scan_args<T>(J[blockIdx.y], which, in, out, blk, total, n);
    const int nb = (n + 1023) / 1024;
    __shared__ T wsum[16], carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + tid;
        const T v = i < nb ? blk[i] : (T)0;
        T x = v;
        for (int o = 1; o < 64; o <<= 1) { const T y = shfl_up_t(x, o); if (lane >= o) x += y; }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        T off = carry_s;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (i < nb) blk[i] = off + x - v;
        __syncthreads();
        if (tid == 1023) carry_s = off + x;
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

template <typename T>
__global__ __launch_bounds__(1024) void scan_add_kernel(const map_job *__restrict__ J, int which)
{
    const T *in; T *out, *blk, *total; int n;
    scan_args<T>(J[blockIdx.y], which, in, out, blk, total, n);
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < n) out[i] += blk[blockIdx.x];
}

// ---- emission into the flat problem -------------------------------------------------------------------
__device__ __forceinline__ void me_poses(const map_job &j, int k, const flat_out &O)
{
    const map_view &M = j.M;
    if (k >= M.max_kf || j.kf_role[k] == 0) return;
    const int p = j.kf_idx[k];
    O.pose_kfid[p] = k;
    O.pose_const[p] = j.kf_role[k] == 2;
    for (int t = 0; t < 7; ++t) O.pose[7 * p + t] = M.kf_pose[7 * k + t];
}

__device__ __forceinline__ void me_lms(const map_job &j, int l, int inv, const flat_out &O)
{
    const map_view &M = j.M;
    if (l >= M.max_lm) return;
    const unsigned long long pi = j.lm_pidx[l];
    if (j.lm_sel[l] == 2) {
        O.bad_lmid[(int)(pi >> 32)] = l;
        j.lm_state_w[l] = M.lm_state[l] & ~OV2_LM_3D;   // MapPoint::isBad() clears is3d_ when it answers true (src/map_point.cpp:219,227)
    }
    if (!j.lm_flag[l]) return;
    const int q = (int)(pi & 0xffffffffull);
    O.lm_lmid[q] = l;
    if (!inv) {
        for (int t = 0; t < 3; ++t) O.lm[3 * q + t] = M.lm_xyz[3 * l + t];
        O.lm_anchor_pose[q] = -1;
        O.lm_anchor_uv[2 * q] = O.lm_anchor_uv[2 * q + 1] = 0.0;
    }
}

// z of (Twc^-1 * p): third row of R' times (p - t); Twc = [t, qx qy qz qw] (Sophus, include/frame.hpp getTcw)
__device__ __forceinline__ double depth_in_kf(const double *T, const double *p)
{
    const double dx = p[0] - T[0], dy = p[1] - T[1], dz = p[2] - T[2];
    double R[9];
    ov2se3::tri_quat_R(T, R);
    return R[2] * dx + R[5] * dy + R[8] * dz;   // third column of R(q) = third row of R'
}

__device__ __forceinline__ void me_res(const map_job &j, int i, int inv, const flat_out &O)
{
    const map_view &M = j.M;
    if (i >= M.n_obs) return;
    int kf, lm;
    if (!obs_live(M, i, kf, lm) || !j.lm_flag[lm] || kf > j.hdr[MH_NMAXKF]) return;
    const int q = (int)(j.lm_pidx[lm] & 0xffffffffull), pj = j.kf_idx[kf];
    const bool stereo = M.obs_flag[i] & OBS_STEREO;
    const double sigma = (double)(1 << M.obs_scale[i]);   // std::pow(2., kp.scale_)
    int o = j.obs_off[i];
    auto put = [&](int type, const double *uv) {
        O.res_type[o] = (unsigned char)type; O.res_pose[o] = pj; O.res_lm[o] = q;
        O.res_uv[2 * o] = uv[0]; O.res_uv[2 * o + 1] = uv[1]; O.res_sigma[o] = sigma;
        O.res_out[o] = 0;
        ++o;
    };
    if (inv && j.lm_anchor[lm] == ANCH_TOP - kf) {
        O.lm[q] = 1.0 / depth_in_kf(M.kf_pose + 7 * kf, M.lm_xyz + 3 * lm);
        O.lm_anchor_pose[q] = pj;
        O.lm_anchor_uv[2 * q] = M.obs_uv[2 * i]; O.lm_anchor_uv[2 * q + 1] = M.obs_uv[2 * i + 1];
        if (stereo) put(OV2_BA_RANCH_INV, M.obs_ruv + 2 * i);
        return;
    }
    put(inv ? OV2_BA_L_INV : OV2_BA_L_XYZ, M.obs_uv + 2 * i);
    if (stereo) put(inv ? OV2_BA_R_INV : OV2_BA_R_XYZ, M.obs_ruv + 2 * i);
}

// one launch: blocks [0, gK) write the poses, [gK, gK + gL) the landmarks and the bad list, the rest the residual
// blocks; block 0 of every map also hands its header to the gathered copy the host reads.  A map whose flat problem does
// not fit its output block emits nothing (the host grows the block and runs the set-up again).
__global__ __launch_bounds__(256) void me_all_kernel(const map_job *__restrict__ J, int gK, int gL, int inv)
{
    const map_job &j = J[blockIdx.y];
    const int blk = blockIdx.x, t = threadIdx.x;
    const int *H = j.hdr;
    size_t off[FO_N];
    const bool aborted = H[MH_ABORT] != 0;
    const size_t need = aborted ? 0 : flat_layout((size_t)H[MH_NPOSE], (size_t)H[MH_NLM], (size_t)H[MH_NRES], (size_t)H[MH_NBAD], inv ? 1 : 3, off);
    const bool fits = need <= j.out_cap;
    if (blk == 0 && t < MH_N) {
        int v = H[t];
        if (t == MH_NEED16) v = (int)(need >> 4);
        if (t == MH_OVER) v = fits ? 0 : 1;
        j.hdr_out[t] = v;
    }
    if (aborted || !fits) return;
    const flat_out O = flat_ptrs(j.out, off);
    if (blk < gK) me_poses(j, blk * 256 + t, O);
    else if (blk < gK + gL) me_lms(j, (blk - gK) * 256 + t, inv, O);
    else me_res(j, (blk - gK - gL) * 256 + t, inv, O);
}

// ---- update stage of Optimizer::localBA (src/optimizer.cpp:741-882) on the tables ---------------------------------
// Inputs: the flat problem where the set-up left it (poses / landmarks now hold the solved states), the per residual block
// outlier flags of the solve, and the set-up's residual blocks per observation row (obs_cnt / obs_off, rows
// [0, last_n_obs) only).  The map may have been edited since the set-up (keyframes or observations appended, observations /
// landmarks removed, isobs_ flipped: the other threads of the reference keep working while the solve runs); everything the
// culling reads -- observers, oldest observer, isobs_, liveness -- is therefore read from the tables as they are NOW, as
// the reference reads its MapPoint objects under the map lock (:789-882).
//
// pass 1, one thread per observation row of the set-up: a flagged LEFT block removes the observation
// (MapManager::removeMapPointObs, :753-764; an observation of the current frame also clears MapPoint::isobs_,
// removeObsFromCurFrameById), a flagged RIGHT block demotes it to mono (Frame::removeStereoKeypointById, :743-751); both put
// the landmark into set_badlmids.  A row that died since the set-up is neither removed again nor reported.  The extra
// blocks [gN, gN + gLM) clear the observer counts / oldest observer of the window's landmarks (local + isBad()) for pass 1b.
__global__ __launch_bounds__(256) void mu_obs_kernel(const map_job *__restrict__ J, int gN, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (j.hdr[MH_ABORT]) return;
    if ((int)blockIdx.x >= gN) {
        const int idx = ((int)blockIdx.x - gN) * 256 + threadIdx.x, NL = j.hdr[MH_NLM], NB = j.hdr[MH_NBAD];
        if (idx >= NL + NB) return;
        const flat_out O = flat_of(j, inv);
        const int l = idx < NL ? O.lm_lmid[idx] : O.bad_lmid[idx - NL];
        j.lm_nobs[l] = 0;
        j.lm_pack[l] = 0ull;            // free after the set-up's scan: the 64-bit oldest observer of pass 1b
        atomicOr(&j.lm_sel[l], 16);     // counted by pass 1b
        return;
    }
    if (!j.outlier || (int)blockIdx.x * 256 >= j.last_n_obs) return;   // uniform per workgroup
    __shared__ int s_cnt[2], s_base[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const flat_out O = flat_of(j, inv);
    bool left = false, right = false;
    const int c = i < j.last_n_obs ? j.obs_cnt[i] : 0;
    if (c) {
        const int o = j.obs_off[i];
        for (int k = 0; k < c; ++k)
            if (j.outlier[o + k]) {
                const int t = O.res_type[o + k];
                if (t == OV2_BA_L_XYZ || t == OV2_BA_L_INV) left = true; else right = true;
            }
    }
    int kf = 0, lm = 0;
    const bool live = (left || right) && obs_live(M, i, kf, lm);
    if (left || right) {
        kf = M.obs_kf[i]; lm = M.obs_lm[i];
        atomicOr(&j.lm_sel[lm], 4);
        // removeObsFromCurFrameById runs whether or not the observation is still there; one observation per (keyframe,
        // landmark) among the set-up's rows: one writer
        if (left && kf == j.cur_kfid) j.lm_state_w[lm] = M.lm_state[lm] & ~OV2_LM_OBS;
    }
    const bool rm = left && live, demote = right && !left && live && (M.obs_flag[i] & OBS_STEREO);
    // the two report lists: ranks inside the workgroup from LDS counters, ONE global atomic per workgroup and list
    // (one per flagged row on the map's header line serialised the whole launch: 1.66 ms for 64 maps of 65 k rows)
    const int rl = rm ? atomicAdd(&s_cnt[0], 1) : 0, rr = demote ? atomicAdd(&s_cnt[1], 1) : 0;
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&j.hdr[threadIdx.x == 0 ? MH_NRM_OBS : MH_NST_OFF], s_cnt[threadIdx.x]);
    __syncthreads();
    if (demote) {
        j.obs_flag_w[i] = M.obs_flag[i] & ~OBS_STEREO;
        O.st_off[s_base[1] + rr] = make_int2(kf, lm);
    }
    if (rm) {
        j.obs_flag_w[i] = 0;
        O.rm_obs[s_base[0] + rl] = make_int2(kf, lm);
    }
}

// pass 1b, one thread per row of the table as it is now (rows appended since the set-up included), after the removals:
// live observers (MapPoint::set_kfids_.size()) and the oldest one (MapPoint::kfid_, which MapPoint::removeKfObs moves to
// the oldest observer left, src/map_point.cpp:124-126) of the window's landmarks.  The oldest observer is packed as
// (ANCH_TOP - kfid) << 32 | row under a 64-bit atomicMax: the row gives the new anchor's pixel (inverse depth).
__global__ __launch_bounds__(256) void mu_recount_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (j.hdr[MH_ABORT] || i >= M.n_obs || !obs_live(M, i, kf, lm) || !(j.lm_sel[lm] & 16)) return;
    atomicAdd(&j.lm_nobs[lm], 1);
    atomicMax(&j.lm_pack[lm], ((unsigned long long)(ANCH_TOP - kf) << 32) | (unsigned)i);
}

// pass 2: blocks [0, gP) write the solved poses of the non-constant keyframes (:767-786); the others take one landmark
// each: the local landmarks (:789-853: isBad / culling / positive depth / new world point) and then, for the members of
// set_badlmids -- the isBad() landmarks of the set-up and every landmark that had a flagged block -- the second
// culling pass (:856-882).  Observers and the oldest observer come from pass 1b, isobs_ / liveness from the tables now.
__global__ __launch_bounds__(256) void mu_apply_kernel(const map_job *__restrict__ J, int gP, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int *H = j.hdr;
    if (H[MH_ABORT]) return;
    const flat_out O = flat_of(j, inv);
    const int blk = blockIdx.x, t = threadIdx.x;
    if (blk < gP) {
        const int p = blk * 256 + t;
        if (p >= H[MH_NPOSE] || O.pose_const[p]) return;
        const int kf = O.pose_kfid[p];
        if (!M.kf_state[kf]) return;
        for (int k = 0; k < 7; ++k) j.kf_pose_w[7 * kf + k] = O.pose[7 * p + k];
        return;
    }
    const int idx = (blk - gP) * 256 + t, NL = H[MH_NLM], NB = H[MH_NBAD];
    if (idx >= NL + NB) return;
    const bool local = idx < NL;
    const int l = local ? O.lm_lmid[idx] : O.bad_lmid[idx - NL];
    int st = M.lm_state[l];
    if (!(st & OV2_LM_ALIVE)) return;   // MapManager::getMapPoint returned nullptr
    const int nobs = j.lm_nobs[l];
    const bool isobs = st & OV2_LM_OBS;
    const unsigned long long oldest = j.lm_pack[l];   // 0: no live observer left
    const int lm_kfid = oldest ? ANCH_TOP - (int)(oldest >> 32) : -1;   // MapPoint::kfid_ = its oldest observer
    auto remove = [&]() { j.lm_state_w[l] = 0; O.rm_lm[atomicAdd(&j.hdr[MH_NRM_LM], 1)] = l; };
    auto is_bad = [&]() {   // MapPoint::isBad (src/map_point.cpp:215-234)
        if ((nobs < 2 && !isobs && (st & OV2_LM_3D)) || (nobs == 0 && !isobs)) { st &= ~OV2_LM_3D; return true; }
        return false;
    };
    auto cull = [&]() { return nobs < 3 && lm_kfid < j.newkf - 3 && !isobs; };   // :808-813, :868-874
    bool in_bad = !local || (j.lm_sel[l] & 4);
    if (local) {
        if (is_bad() || cull()) { remove(); return; }
        double wpt[3];
        bool have = true;
        if (inv) {
            const double rho = O.lm[idx], zanch = 1.0 / rho;
            if (zanch <= 0.0) { remove(); return; }
            // the landmark's anchor keyframe NOW (:822): the set-up's unless its observation went away; the solved inverse
            // depth is applied to that keyframe's pose and pixel, as the reference does
            const int r = (int)(oldest & 0xffffffffull), akf = oldest ? M.obs_kf[r] : -1;
            const int a = akf >= 0 && j.kf_role[akf] ? j.kf_idx[akf] : -1;
            if (a < 0 || !M.kf_state[akf]) { in_bad = true; have = false; }   // not in map_local_pkfs / pkfanch == nullptr (:822-848)
            else {
                const double u = M.obs_uv[2 * r], v = M.obs_uv[2 * r + 1];
                const double cam[3] = {zanch * (u - j.K[2]) / j.K[0], zanch * (v - j.K[3]) / j.K[1], zanch};
                ov2se3::tri_apply(O.pose + 7 * a, cam, wpt);   // Twc * cam
            }
        } else {
            wpt[0] = O.lm[3 * idx]; wpt[1] = O.lm[3 * idx + 1]; wpt[2] = O.lm[3 * idx + 2];
        }
        if (have) {   // MapManager::updateMapPoint: a 2D point turns 3D with its keypoints, then MapPoint::setPoint
            j.lm_xyz_w[3 * l] = wpt[0]; j.lm_xyz_w[3 * l + 1] = wpt[1]; j.lm_xyz_w[3 * l + 2] = wpt[2];
            st |= OV2_LM_3D | OV2_LM_KP3D;
        }
    }
    if (in_bad && (is_bad() || cull())) { remove(); return; }
    if (st != (int)M.lm_state[l]) j.lm_state_w[l] = (unsigned char)st;
}

// ---- Mapper::triangulateTemporal (src/mapper.cpp:191-344) on the tables ---------------------------------------------
// The new keyframe's 2D keypoints are the live rows (newkf, l) of landmarks that are alive and neither OV2_LM_3D nor
// OV2_LM_KP3D.  Header of the stage (its own block, cleared per call): what ov2_map_temporal reports.
enum { TH_SELECTED = 0, TH_CANDIDATES, TH_GOOD, TH_REMOVED };

__device__ __forceinline__ bool lm_is_2d(const map_view &M, int lm) { return !(M.lm_state[lm] & (OV2_LM_3D | OV2_LM_KP3D)); }

// observer scan: MapPoint::set_kfids_.size(), its *begin() (order-independent integer atomics) and the row of the new keyframe
__global__ __launch_bounds__(256) void mt_observers_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i >= M.n_obs || !obs_live(M, i, kf, lm) || !lm_is_2d(M, lm)) return;
    atomicAdd(&j.tt_nobs[lm], 1);
    atomicMax(&j.tt_old[lm], ANCH_TOP - kf);       // the smallest kfid wins
    if (kf == j.newkf) j.tt_nrow[lm] = i + 1;      // one live row per (keyframe, landmark): one writer
}

// row scan: the row of the oldest observer of every landmark the new keyframe holds in 2D
__global__ __launch_bounds__(256) void mt_rows_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i >= M.n_obs || !obs_live(M, i, kf, lm) || !lm_is_2d(M, lm) || !j.tt_nrow[lm]) return;
    if (j.tt_old[lm] == ANCH_TOP - kf) j.tt_arow[lm] = i;
}

// SE3::inverse / SE3::operator* of the host mirror (ov2_host.cpp), so that Tcicj = Tciw * Twcj rounds as it does there
__device__ __forceinline__ void se3_inverse(const double *T, double out[7])
{
    double R[9];
    ov2se3::pose_R(T, R);
    out[0] = -(R[0] * T[0] + R[3] * T[1] + R[6] * T[2]);
    out[1] = -(R[1] * T[0] + R[4] * T[1] + R[7] * T[2]);
    out[2] = -(R[2] * T[0] + R[5] * T[1] + R[8] * T[2]);
    const double n = __dsqrt_rn(T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6]);
    out[3] = -T[3] / n; out[4] = -T[4] / n; out[5] = -T[5] / n; out[6] = T[6] / n;
}

__device__ __forceinline__ void se3_mul(const double *A, const double *B, double out[7])
{
    double Ra[9], Rb[9], R[9];
    ov2se3::pose_R(A, Ra);
    ov2se3::pose_R(B, Rb);
    R[0] = Ra[0] * Rb[0] + Ra[1] * Rb[3] + Ra[2] * Rb[6]; R[1] = Ra[0] * Rb[1] + Ra[1] * Rb[4] + Ra[2] * Rb[7];
    R[2] = Ra[0] * Rb[2] + Ra[1] * Rb[5] + Ra[2] * Rb[8]; R[3] = Ra[3] * Rb[0] + Ra[4] * Rb[3] + Ra[5] * Rb[6];
    R[4] = Ra[3] * Rb[1] + Ra[4] * Rb[4] + Ra[5] * Rb[7]; R[5] = Ra[3] * Rb[2] + Ra[4] * Rb[5] + Ra[5] * Rb[8];
    R[6] = Ra[6] * Rb[0] + Ra[7] * Rb[3] + Ra[8] * Rb[6]; R[7] = Ra[6] * Rb[1] + Ra[7] * Rb[4] + Ra[8] * Rb[7];
    R[8] = Ra[6] * Rb[2] + Ra[7] * Rb[5] + Ra[8] * Rb[8];
    out[0] = Ra[0] * B[0] + Ra[1] * B[1] + Ra[2] * B[2] + A[0];
    out[1] = Ra[3] * B[0] + Ra[4] * B[1] + Ra[5] * B[2] + A[1];
    out[2] = Ra[6] * B[0] + Ra[7] * B[1] + Ra[8] * B[2] + A[2];
    ov2se3::rot_to_quat(R, out + 3);
}

// Frame::computeKeypoint (src/frame.cpp:246-254) for a pinhole camera: unpx as the float the host keeps, bearing iK * [unpx, 1] normalised
__device__ __forceinline__ void bearing_of(const double K[4], const double *uv, float &u, float &v, double bv[3])
{
    u = (float)uv[0]; v = (float)uv[1];
    const double x = ((double)u - K[2]) / K[0], y = ((double)v - K[3]) / K[1];
    const double nrm = __dsqrt_rn(x * x + y * y + 1.0 * 1.0);
    bv[0] = x / nrm; bv[1] = y / nrm; bv[2] = 1.0 / nrm;
}

// candidates + apply, one lane per landmark: the reference's skips (:258-289), then tri_kernel's arithmetic in its order
// (tri_pair.h) and the bookkeeping of its verdict (:310-333).  Every landmark is read and written by its own lane only.
__global__ __launch_bounds__(256) void mt_tri_kernel(const map_job *__restrict__ J, int stereo, float max_err)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if ((int)blockIdx.x * 256 >= M.max_lm) return;   // uniform per workgroup
    __shared__ int s_cnt[4], s_base[2];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int nr = l < M.max_lm ? j.tt_nrow[l] : 0;
    bool cand = false, good = false, rm = false;
    double wpt[3] = {0., 0., 0.}, invdepth = 0.;
    const int oldkf = nr ? ANCH_TOP - j.tt_old[l] : -1;
    if (nr && j.tt_nobs[l] >= 2 && oldkf != j.newkf) {   // :258-266 (the oldest observer is alive and holds the keypoint: obs_live)
        double Tciw[7], T[7];
        se3_inverse(M.kf_pose + 7 * (size_t)oldkf, Tciw);
        se3_mul(Tciw, M.kf_pose + 7 * (size_t)j.newkf, T);   // Tcicj (:278-279)
        if (!(stereo && __dsqrt_rn(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]) < 0.01)) {   // :287
            cand = true;
            float ua, va, ub, vb;
            double f1[3], f2[3], f2u[3], R[9], X[3];
            const int ar = min(max(j.tt_arow[l], 0), M.n_obs - 1);   // written by the row scan for every such landmark; clamped all the same
            bearing_of(j.K, M.obs_uv + 2 * (size_t)ar, ua, va, f1);
            bearing_of(j.K, M.obs_uv + 2 * (size_t)(nr - 1), ub, vb, f2);
            ov2se3::tri_quat_R(T, R);
            ov2tri::rotate(R, f2, f2u);
            const double parallax = ov2tri::parallax_px(j.K, f2u, ua, va);
            ov2tri::midpoint(T, f1, f2u, X);
            const int st = ov2tri::gates(T, R, X, j.K, j.K, ua, va, ub, vb, max_err);
            if (st == OV2_TRI_OK) {
                good = true;
                ov2se3::tri_apply(M.kf_pose + 7 * (size_t)oldkf, X, wpt);
                invdepth = 1. / X[2];
            } else rm = parallax > 20.;
        }
    }
    if (nr) atomicAdd(&s_cnt[TH_SELECTED], 1);
    if (cand) atomicAdd(&s_cnt[TH_CANDIDATES], 1);
    const int rg = good ? atomicAdd(&s_cnt[TH_GOOD], 1) : 0, rr = rm ? atomicAdd(&s_cnt[TH_REMOVED], 1) : 0;
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) {   // one global atomic per workgroup and counter
        const int base = atomicAdd(&j.hdr[threadIdx.x], s_cnt[threadIdx.x]);
        if (threadIdx.x >= TH_GOOD) s_base[threadIdx.x - TH_GOOD] = base;
    }
    __syncthreads();
    if (good) {   // MapManager::updateMapPoint: the point turns 3D with its keypoints
        j.lm_xyz_w[3 * (size_t)l] = wpt[0]; j.lm_xyz_w[3 * (size_t)l + 1] = wpt[1]; j.lm_xyz_w[3 * (size_t)l + 2] = wpt[2];
        j.lm_state_w[l] = M.lm_state[l] | OV2_LM_3D | OV2_LM_KP3D;
        const int o = s_base[0] + rg;
        j.tt_good_lmid[o] = l; j.tt_good_inv[o] = invdepth;
        j.tt_good_wpt[3 * (size_t)o] = wpt[0]; j.tt_good_wpt[3 * (size_t)o + 1] = wpt[1]; j.tt_good_wpt[3 * (size_t)o + 2] = wpt[2];
    }
    if (rm) {     // MapManager::removeMapPointObs(lmid, newkf)
        j.obs_flag_w[nr - 1] = 0;
        j.tt_rm_lmid[s_base[1] + rr] = l;
    }
}

// ---- Mapper::triangulateStereo (src/mapper.cpp:346-461) on the tables ------------------------------------------------
// The intake first: the Frame::updateKeypointStereo loop that ends MapManager::stereoMatching (src/map_manager.cpp:583-604)
// from the matcher's device arrays.  Scatter: the landmark remembers the last entry that names it with a non-zero status
// (atomicMax: list order decides, as it does in map_edit_obs_kernel); an id outside [0, max_lm) indexes nothing.
__global__ __launch_bounds__(256) void si_scatter_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j.si_n || !j.si_status[i]) return;
    const int l = j.si_lmid[i];
    if (l < 0 || l >= j.M.max_lm) return;
    atomicMax(&j.ts_mark[l], i + 1);
}

// row scan: the live row (kfid, l) of a marked landmark takes the flag and the undistorted right pixel, held as the double of
// the float Frame::updateKeypointStereo keeps (src/frame.cpp:405-433)
__global__ __launch_bounds__(256) void si_rows_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M.n_obs || !(M.obs_flag[i] & OBS_ALIVE) || M.obs_kf[i] != j.newkf) return;
    const int l = M.obs_lm[i];
    const int e = (l >= 0 && l < M.max_lm) ? j.ts_mark[l] : 0;
    if (!e) return;
    float ru, rv;
    ov2_cam_undistort(j.si_cam, j.si_rxy[2 * (size_t)(e - 1)], j.si_rxy[2 * (size_t)(e - 1) + 1], ru, rv);
    j.obs_flag_w[i] = M.obs_flag[i] | OBS_STEREO;
    j.obs_ruv_w[2 * (size_t)i] = (double)ru; j.obs_ruv_w[2 * (size_t)i + 1] = (double)rv;
}

// Header of the stage (its own block, cleared per call): what ov2_map_stereo_tri reports.
enum { SH_SELECTED = 0, SH_GOOD, SH_DEMOTED };

// one lane per observation row: the stereo rows of the new keyframe whose landmark is still 2D (:383), tri_kernel's
// arithmetic in its order (tri_pair.h) and the bookkeeping of its verdict (:413-450).  One live row per (keyframe, landmark):
// every landmark and every row is read and written by one lane only.
__global__ __launch_bounds__(256) void mst_tri_kernel(const map_job *__restrict__ J, float max_err)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if ((int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    __shared__ int s_cnt[3], s_base[2];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = -1, l = 0;
    const bool sel = i < M.n_obs && obs_live(M, i, kf, l) && kf == j.newkf && (M.obs_flag[i] & OBS_STEREO) && lm_is_2d(M, l);
    int st = OV2_TRI_OK;
    double wpt[3] = {0., 0., 0.}, invdepth = 0.;
    if (sel) {
        float ua, va, ub, vb;
        double f1[3], f2[3], f2u[3], R[9], X[3];
        bearing_of(j.K, M.obs_uv + 2 * (size_t)i, ua, va, f1);
        bearing_of(j.st_Kr, M.obs_ruv + 2 * (size_t)i, ub, vb, f2);
        ov2se3::tri_quat_R(j.st_Tlr, R);
        ov2tri::rotate(R, f2, f2u);
        bool have = true;
        if (j.st_rect) have = ov2tri::rectified(j.st_Tlr, j.K, ua, va, ub, X);   // :410-422
        else ov2tri::midpoint(j.st_Tlr, f1, f2u, X);                             // :424
        st = have ? ov2tri::gates(j.st_Tlr, R, X, j.K, j.st_Kr, ua, va, ub, vb, max_err) : OV2_TRI_NEG_DISP;
        if (st == OV2_TRI_OK) {
            ov2se3::tri_apply(M.kf_pose + 7 * (size_t)j.newkf, X, wpt);          // Frame::projCamToWorld (:448)
            invdepth = 1. / X[2];
        }
    }
    const bool good = sel && st == OV2_TRI_OK, dem = sel && st != OV2_TRI_OK;
    if (sel) atomicAdd(&s_cnt[SH_SELECTED], 1);
    const int rg = good ? atomicAdd(&s_cnt[SH_GOOD], 1) : 0, rd = dem ? atomicAdd(&s_cnt[SH_DEMOTED], 1) : 0;
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) {   // one global atomic per workgroup and counter
        const int base = atomicAdd(&j.hdr[threadIdx.x], s_cnt[threadIdx.x]);
        if (threadIdx.x >= SH_GOOD) s_base[threadIdx.x - SH_GOOD] = base;
    }
    __syncthreads();
    if (good) {   // MapManager::updateMapPoint (:450): the point turns 3D with its keypoints
        j.lm_xyz_w[3 * (size_t)l] = wpt[0]; j.lm_xyz_w[3 * (size_t)l + 1] = wpt[1]; j.lm_xyz_w[3 * (size_t)l + 2] = wpt[2];
        j.lm_state_w[l] = M.lm_state[l] | OV2_LM_3D | OV2_LM_KP3D;
        const int o = s_base[0] + rg;
        if (o < M.max_lm) {   // always, with one live row per (keyframe, landmark); the lists hold max_lm entries
            j.ts_good_lmid[o] = l; j.ts_good_inv[o] = invdepth;
            j.ts_good_wpt[3 * (size_t)o] = wpt[0]; j.ts_good_wpt[3 * (size_t)o + 1] = wpt[1]; j.ts_good_wpt[3 * (size_t)o + 2] = wpt[2];
        }
    }
    if (dem) {    // Frame::removeStereoKeypointById (:414, :431, :443): the right pixel stays where it is
        j.obs_flag_w[i] = M.obs_flag[i] & ~OBS_STEREO;
        const int o = s_base[1] + rd;
        if (o < M.max_lm) { j.ts_dem_lmid[o] = l; j.ts_why[o] = (unsigned char)st; }
    }
}

// ---- Estimator::mapFiltering (src/estimator.cpp:101-183) on the tables -----------------------------------------------
// Rank of a lane among the lanes of its wave that hold the same key, and their number: one atomic per wave and key where
// one per row would serialise on the keyframe's counter (rows of a keyframe are mostly adjacent).  All lanes of the wave
// must call it; `first` is the lowest lane of the key (the lane's own when it is off), the one to issue the atomic.
__device__ __forceinline__ int wave_rank_by_key(bool on, int key, int &count, int &first_lane)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(on);
    int rank = 0;
    count = 0; first_lane = lane;
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, first);
        const unsigned long long same = __ballot(on && key == k0);
        if (on && key == k0) {
            rank = __popcll(same & ((1ull << lane) - 1ull));
            count = __popcll(same);
            first_lane = first;
        }
        todo &= ~same;
    }
    return rank;
}

// row scan: MapPoint::set_kfids_.size() per landmark, the landmarks of the new keyframe, live rows and 3D rows
// (Frame::nb3dkps_) per keyframe
__global__ __launch_bounds__(256) void mf_count_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.fl_active || (int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    const bool live = i < M.n_obs && obs_live(M, i, kf, lm);
    const bool is3d = live && (M.lm_state[lm] & OV2_LM_KP3D);
    const int lane = threadIdx.x & 63;
    int n, n3, first, first3;
    wave_rank_by_key(live, kf, n, first);
    wave_rank_by_key(is3d, kf, n3, first3);
    if (live && lane == first) atomicAdd(&j.fl_cnt[kf], n);
    if (is3d && lane == first3) atomicAdd(&j.fl_n3d[kf], n3);
    if (!live) return;
    atomicAdd(&j.fl_nobs[lm], 1);
    if (kf == j.newkf) j.fl_new[lm] = 1;
}

// covisibility with the new keyframe (MapManager::updateFrameCovisibility, as ms_cov_kernel recounts it) and the scatter of
// the counting sort: row i joins the rows of its keyframe, in any order (only integer sums are taken over them)
__global__ __launch_bounds__(256) void mf_index_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.fl_active || (int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    const bool live = i < M.n_obs && obs_live(M, i, kf, lm);
    const bool cov = live && kf != j.newkf && j.fl_new[lm];
    const int lane = threadIdx.x & 63;
    int n, nc, first, firstc;
    const int rank = wave_rank_by_key(live, kf, n, first);
    wave_rank_by_key(cov, kf, nc, firstc);
    if (cov && lane == firstc) atomicAdd(&j.fl_cov[kf], nc);
    int base = (live && lane == first) ? atomicAdd(&j.fl_fill[kf], n) : 0;
    base = __shfl(base, first);
    // fl_start[kf] + fl_cnt[kf] <= FH_ROWS <= n_obs <= max_obs: the slot lies inside fl_rows
    if (live) j.fl_rows[j.fl_start[kf] + base + rank] = i;
}

// One workgroup per map walks the candidates newest -> oldest (:119-179); its tail hands the header and the removed list to
// the gathered copy.  The observer counts and landmark states the walk edits live in global memory and are read again by
// other lanes for the next candidate: they go through device-scope atomics, and a barrier separates a candidate's edits
// from the next candidate's reads.  Everything that decides the control flow is uniform over the workgroup.
#define MF_THREADS 256
__device__ __forceinline__ int ld_int(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_u8(const unsigned char *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u8(unsigned char *p, int v) { __hip_atomic_store(p, (unsigned char)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(MF_THREADS) void mf_walk_kernel(const map_job *__restrict__ J, int nmin_cov, float ratio_th, int list_cap)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ int s_good[MF_THREADS / 64], s_tot[MF_THREADS / 64], s_unset;
    int ncand = 0, nrem = 0, nfew = 0;   // the same in every lane
    if (tid == 0) s_unset = 0;
    __syncthreads();
    if (j.fl_active) {
        for (int k = min(M.max_kf, j.newkf) - 1; k > 0; --k) {
            if (!M.kf_state[k] || j.fl_cov[k] < 1) continue;   // not in the map / not in newkf's covisibility map
            ++ncand;
            const int cnt = j.fl_cnt[k];
            const int *rows = j.fl_rows + j.fl_start[k];
            bool remove = j.fl_n3d[k] < nmin_cov / 2;           // :139-143
            if (remove) ++nfew;
            else {
                int good = 0, tot = 0;
                for (int t = tid; t < cnt; t += MF_THREADS) {   // Frame::getKeypoints3d of k (:147-170)
                    const int lm = M.obs_lm[rows[t]];
                    const int st = ld_u8(j.lm_state_w + lm);
                    if (!(st & OV2_LM_KP3D)) continue;
                    const int nobs = ld_int(j.fl_nobs + lm);
                    if (nobs < 2 && !(st & OV2_LM_OBS) && (st & OV2_LM_3D)) {   // MapPoint::isBad: is3d_ goes, the point is not counted
                        st_u8(j.lm_state_w + lm, st & ~OV2_LM_3D);
                        j.fl_unset[atomicAdd(&s_unset, 1)] = lm;                  // a landmark turns bad once: at most max_lm entries
                        continue;
                    }
                    ++tot;
                    good += nobs > 4;
                }
                for (int o = 32; o; o >>= 1) { good += __shfl_xor(good, o); tot += __shfl_xor(tot, o); }
                if (lane == 0) { s_good[wv] = good; s_tot[wv] = tot; }
                __syncthreads();
                good = tot = 0;
                for (int w = 0; w < MF_THREADS / 64; ++w) { good += s_good[w]; tot += s_tot[w]; }
                // float ratio = (float)nbgoodobs / nbtot; if (ratio > fkf_filtering_ratio_): 0 / 0 is NaN and compares false (:171-172)
                const float ratio = (float)good / (float)tot;
                remove = ratio > ratio_th;
            }
            if (remove) {   // MapManager::removeKeyframe: every keypoint's map point loses the observer, 2D ones included
                for (int t = tid; t < cnt; t += MF_THREADS) {
                    const int lm = M.obs_lm[rows[t]];
                    if (atomicSub(&j.fl_nobs[lm], 1) == 1) {   // no observer left: no keypoint left to carry Keypoint::is3d_
                        const int st = ld_u8(j.lm_state_w + lm);
                        if (!(st & OV2_LM_3D) && (st & OV2_LM_KP3D)) st_u8(j.lm_state_w + lm, st & ~OV2_LM_KP3D);
                    }
                }
                if (tid == 0) {
                    j.kf_state_w[k] = 0;
                    if (nrem < list_cap) j.hdr_out[MH_N + nrem] = k;
                }
                ++nrem;
            }
            __syncthreads();   // the decrements and state edits before the next candidate's reads; s_good / s_tot free again
        }
    }
    if (tid == 0) {
        int *H = j.hdr_out;
        for (int t = 0; t < MH_N; ++t) H[t] = 0;
        H[FH_CANDIDATES] = ncand; H[FH_REMOVED] = nrem; H[FH_FEW3D] = nfew; H[FH_UNSET3D] = s_unset;
    }
}

// ---- the local map of a new keyframe: MapManager::updateFrameCovisibility (src/map_manager.cpp:117-193) and the extension of
// Mapper::matchingToLocalMap (src/mapper.cpp:475-517) on the tables and the per-keyframe id sets ------------------------------
// row scan: Obs(k), the landmarks with a live row in the new keyframe (2D and 3D keypoints alike, Frame::getKeypoints)
__global__ __launch_bounds__(256) void li_obs_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i >= M.n_obs || !obs_live(M, i, kf, lm)) return;
    if (kf == j.newkf) j.ls_obs[lm] = 1;   // every writer stores the same value
}

// row scan: cov[j] as ms_cov_kernel counts it, one atomic per wave and keyframe (rows of a keyframe are mostly adjacent: a
// wave would otherwise queue 64 adds on one counter), and the smallest covisible kfid beside it
__global__ __launch_bounds__(256) void li_cov_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if ((int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    const bool live = i < M.n_obs && obs_live(M, i, kf, lm);
    const bool cov = live && kf != j.newkf && j.ls_obs[lm];
    int n, first;
    wave_rank_by_key(cov, kf, n, first);
    if (cov && (int)(threadIdx.x & 63) == first) {
        atomicAdd(&j.ls_cov[kf], n);
        atomicMax(&j.hdr[LH_OLDMAX], ANCH_TOP - kf);
    }
}

// row scan: S, the Frame::getKeypoints3d landmarks of the covisible keyframes that the new keyframe does not observe.  A
// landmark is marked by the first of its rows to arrive (an exchange on its word; rows that find the mark set pass by
// without an atomic) and counted there: one add per wave, behind a ballot
__global__ __launch_bounds__(256) void li_fresh_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if ((int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    const bool live = i < M.n_obs && obs_live(M, i, kf, lm);
    const bool cand = live && kf != j.newkf && j.ls_cov[kf] > 0 && (M.lm_state[lm] & OV2_LM_KP3D) && !j.ls_obs[lm];
    bool first = false;
    if (cand && !ld_int(j.ls_mark + lm)) first = atomicExch(&j.ls_mark[lm], 1) == 0;
    const unsigned long long bal = __ballot(first);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&j.hdr[LH_NFRESH], __popcll(bal));
}

// marks the ids of a stored set (pool[start .. start + count)); returns how many this lane marked first
__device__ __forceinline__ int li_mark_list(const map_job &j, int start, int count)
{
    int added = 0;
    for (int t = threadIdx.x; t < count; t += 1024) {
        const int id = j.ls_pool[start + t];
        if ((unsigned)id < (unsigned)j.M.max_lm && atomicExch(&j.ls_mark[id], 1) == 0) ++added;
    }
    return added;
}

// One workgroup per map: the covisibility lists in ascending kfid (a block scan over the keyframes, 1024 per step), then the
// two rules on the device counts -- the store rule of updateFrameCovisibility (:185-189) over the stored set of the new
// keyframe, the size gate of matchingToLocalMap (:481-497) over the stored set of the oldest covisible keyframe -- each
// marking the ids it lets in.  Everything that decides the control flow is uniform over the workgroup.
__global__ __launch_bounds__(1024) void li_lists_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const int max_kf = j.M.max_kf;
    __shared__ int wsum[16], carry_s, s_added;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int *out_kf = j.hdr_out + MH_N, *out_score = out_kf + j.ls_kcap;
    if (tid == 0) { carry_s = 0; s_added = 0; }
    __syncthreads();
    for (int base = 0; base < max_kf; base += 1024) {
        const int k = base + tid;
        const int score = k < max_kf ? j.ls_cov[k] : 0;
        const int f = score > 0 ? 1 : 0;
        int x = f;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int off = carry_s;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        if (f && off + x - 1 < j.ls_kcap) { out_kf[off + x - 1] = k; out_score[off + x - 1] = score; }
        __syncthreads();
        if (tid == 1023) carry_s = off + x;
        __syncthreads();
    }
    const int ncov = carry_s;
    const int nfresh = j.hdr[LH_NFRESH];
    const int oldest = ncov ? ANCH_TOP - j.hdr[LH_OLDMAX] : -1;
    const int nold = j.ls_count[j.newkf];
    const bool swapped = 2ll * nfresh > (long long)nold;
    int added = swapped ? 0 : li_mark_list(j, j.ls_start[j.newkf], nold);
    for (int o = 32; o; o >>= 1) added += __shfl_xor(added, o);
    if (lane == 0 && added) atomicAdd(&s_added, added);
    __syncthreads();
    const bool extended = j.ls_extend && ncov > 0 && nfresh + s_added < j.ls_nmax;
    if (extended) (void)li_mark_list(j, j.ls_start[oldest], j.ls_count[oldest]);   // a keyframe without a stored set has count 0
    if (tid == 0) {
        j.hdr[LH_NCOV] = ncov; j.hdr[LH_OLDEST] = oldest; j.hdr[LH_SWAPPED] = swapped; j.hdr[LH_EXTENDED] = extended;
    }
}

// the marked landmarks in ascending lmid, to the pool segment of the new keyframe's set and to the gathered copy; the first
// thread hands the header over and enters the set into the per-keyframe tables
__global__ __launch_bounds__(256) void li_emit_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < j.M.max_lm && j.ls_mark[l]) {
        const int pos = j.ls_pos[l];
        if (pos < j.ls_room) {   // ls_room entries are reserved in the pool and in the gathered copy (never exceeded: the host sized it)
            j.ls_pool[j.ls_pool_off + pos] = l;
            j.hdr_out[MH_N + 2 * j.ls_kcap + pos] = l;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int t = 0; t < MH_N; ++t) j.hdr_out[t] = j.hdr[t];
        j.ls_start[j.newkf] = j.ls_pool_off;
        j.ls_count[j.newkf] = min(j.hdr[LH_NLOCAL], j.ls_room);
    }
}

// ---- MapManager::mergeMapPoints (src/map_manager.cpp:801-882) on the tables ---------------------------------------------
// The pairs of a map are applied one after the other, each against the tables as the pairs before it left them.  Three
// scans build an index of the rows of the landmarks the list names (mark, count, scan, scatter: a counting sort by
// landmark, as the keyframe filter sorts by keyframe), then one workgroup per map walks the list.  A landmark owns the
// segment of its rows as they stood before the call; a merged `prev` hands its segments on: its chain is linked behind
// the chain of `new`, so a later pair that names `new` finds the adopted rows too and passes over rows whose label has
// moved on (conflict rows keep the dead label).  A pair costs the rows of its two chains, never the table.
__device__ __forceinline__ void st_int(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// pairs of the segment that count: all of them, or the device-side count clamped to the segment
__device__ __forceinline__ int mg_npairs(const map_job &j)
{
    return j.mg_n_dev ? min(j.mg_seg, max(*j.mg_n_dev, 0)) : j.mg_seg;
}

__global__ __launch_bounds__(256) void mg_mark_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (j.gt_on) {   // the match gather names the landmarks of its keypoints and candidates; an id out of range names none
        if (i >= j.gt_nkp + j.gt_ncand) return;
        const int l = i < j.gt_nkp ? j.gt_kp_lmid[i] : j.gt_cand_lmid[i - j.gt_nkp];
        if ((unsigned)l < (unsigned)j.M.max_lm) j.mg_mark[l] = 1;
        return;
    }
    if (i >= mg_npairs(j)) return;
    if (j.sb_on) {   // structure-only BA names the landmarks of its list; the first place an id stands at is the one that enters
        const int l = j.mg_new[i];
        if ((j.sb_status && j.sb_status[i] != OV2_MERGE_DONE) || (unsigned)l >= (unsigned)j.M.max_lm) return;
        j.mg_mark[l] = 1;
        atomicMax(&j.mg_next[l], ANCH_TOP - i);   // 0 = not listed: the array lives in the cleared block
        return;
    }
    const int p = j.mg_prev[i], n = j.mg_new[i];
    if ((unsigned)p >= (unsigned)j.M.max_lm || (unsigned)n >= (unsigned)j.M.max_lm) return;   // the walk skips the pair
    j.mg_mark[p] = 1; j.mg_mark[n] = 1;
}

__global__ __launch_bounds__(256) void mg_count_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.mg_seg || (int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    if (i < M.n_obs && obs_live(M, i, kf, lm) && j.mg_mark[lm]) atomicAdd(&j.mg_cnt[lm], 1);
}

// row i joins the rows of its landmark, in any order (the walk's edits do not depend on it)
__global__ __launch_bounds__(256) void mg_index_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.mg_seg || (int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf = 0, lm = 0;
    // mg_start[lm] + mg_cnt[lm] <= GH_ROWS <= n_obs <= max_obs: the slot lies inside mg_rows
    if (i < M.n_obs && obs_live(M, i, kf, lm) && j.mg_mark[lm]) j.mg_rows[j.mg_start[lm] + atomicAdd(&j.mg_fill[lm], 1)] = i;
}

// One workgroup per map walks its pairs in list order; its tail writes the header into the gathered copy.  Labels, landmark
// states, stamps and links that a pair edits are read again by other lanes for the next pair: they go through device-scope
// atomics, and barriers separate the stamps of `new` from the test of `prev`'s rows, and a pair's edits from the next pair's
// reads.  Everything that decides the control flow (the pair, its status, the chains) is uniform over the workgroup.
#define MG_THREADS 256
__global__ __launch_bounds__(MG_THREADS) void mg_walk_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ int s_moved[MG_THREADS / 64], s_conf[MG_THREADS / 64];
    const int np = mg_npairs(j);
    int nmerged = 0, nskipped = 0;   // the same in every lane
    int moved = 0, conflict = 0;     // this lane's rows
    for (int i = 0; i < np; ++i) {
        const int p = j.mg_prev[i], n = j.mg_new[i];
        int status = OV2_MERGE_DONE, sn = 0;
        if ((unsigned)p >= (unsigned)M.max_lm || (unsigned)n >= (unsigned)M.max_lm) status = OV2_MERGE_SKIP_RANGE;
        else if (p == n) status = OV2_MERGE_SKIP_SAME;
        else {
            sn = ld_u8(j.lm_state_w + n);
            if (!(ld_u8(j.lm_state_w + p) & OV2_LM_ALIVE)) status = OV2_MERGE_SKIP_PREV_DEAD;
            else if (!(sn & OV2_LM_ALIVE)) status = OV2_MERGE_SKIP_NEW_DEAD;
            else if (!(sn & OV2_LM_3D)) status = OV2_MERGE_SKIP_NEW_NOT3D;   // :812-827
        }
        if (tid == 0 && j.mg_status) j.mg_status[i] = (unsigned char)status;
        if (status != OV2_MERGE_DONE) { ++nskipped; continue; }   // nothing was edited: no barrier owed
        ++nmerged;
        // the keyframes that hold `new` (Frame::mapkps_.count(newlmid)); both landmarks are alive, so a row of their chains
        // that still carries the label is a live row
        int tail = n;
        for (int s = n; s >= 0; s = ld_int(j.mg_next + s) - 1) {
            tail = s;
            const int *rows = j.mg_rows + j.mg_start[s];
            const int cnt = j.mg_cnt[s];
            for (int t = tid; t < cnt; t += MG_THREADS) {
                const int r = rows[t];
                if (ld_int(j.obs_lm_w + r) == n) {
                    if (j.mg_srow) st_int(j.mg_srow + M.obs_kf[r], r);   // read only behind a matching stamp
                    st_int(j.mg_stamp + M.obs_kf[r], i + 1);
                }
            }
        }
        __syncthreads();
        // Frame::updateKeypointId(prevlmid, newlmid) per observer of `prev`: false where the keyframe holds `new` already
        for (int s = p; s >= 0; s = ld_int(j.mg_next + s) - 1) {
            const int *rows = j.mg_rows + j.mg_start[s];
            const int cnt = j.mg_cnt[s];
            for (int t = tid; t < cnt; t += MG_THREADS) {
                const int r = rows[t];
                if (ld_int(j.obs_lm_w + r) != p) continue;
                if (ld_int(j.mg_stamp + M.obs_kf[r]) == i + 1) {
                    ++conflict;
                    // MapPoint::addDesc(kfid, prev's descriptor) returns early where `new` has one for the keyframe
                    // (src/map_manager.cpp:854-856, src/map_point.cpp:164-171): `new`'s row takes it only if it has none.  A
                    // keyframe holds one live row of `prev`, so one lane writes a given row of `new`.
                    if (j.obs_hasdesc_w && ld_u8(j.obs_hasdesc_w + r)) {
                        const int r2 = ld_int(j.mg_srow + M.obs_kf[r]);
                        if (!ld_u8(j.obs_hasdesc_w + r2)) {
                            j.obs_desc_w[2 * (size_t)r2] = j.obs_desc_w[2 * (size_t)r];
                            j.obs_desc_w[2 * (size_t)r2 + 1] = j.obs_desc_w[2 * (size_t)r + 1];
                            __threadfence();   // the descriptor before its flag, for the lanes that read both for a later pair
                            st_u8(j.obs_hasdesc_w + r2, 1);
                        }
                    }
                } else { st_int(j.obs_lm_w + r, n); ++moved; }
            }
        }
        if (tid == 0) {
            st_int(j.mg_next + tail, p + 1);   // the chains are disjoint: no lane reads this link before the barrier
            st_u8(j.lm_state_w + p, 0);        // map_plms_.erase(prevlmid)
            if (j.mg_cur && j.mg_cur[i]) st_u8(j.lm_state_w + n, sn | OV2_LM_OBS);   // setMapPointObs(newlmid), :860-866
        }
        __syncthreads();
    }
    if (j.mg_status)   // the pairs of the segment beyond the device-side count
        for (int t = np + tid; t < j.mg_seg; t += MG_THREADS) j.mg_status[t] = OV2_MERGE_NOT_RUN;
    for (int o = 32; o; o >>= 1) { moved += __shfl_xor(moved, o); conflict += __shfl_xor(conflict, o); }
    if (lane == 0) { s_moved[wv] = moved; s_conf[wv] = conflict; }
    __syncthreads();
    if (tid == 0) {
        moved = conflict = 0;
        for (int w = 0; w < MG_THREADS / 64; ++w) { moved += s_moved[w]; conflict += s_conf[w]; }
        int *H = j.hdr_out;
        for (int t = 0; t < MH_N; ++t) H[t] = 0;
        H[GH_PAIRS] = np; H[GH_MERGED] = nmerged; H[GH_SKIPPED] = nskipped; H[GH_MOVED] = moved; H[GH_CONFLICT] = conflict;
    }
}

// ---- structure-only BA: Optimizer::structureOnlyBA (src/optimizer.cpp:2594-2781) on the tables ---------------------------------
// The merge stage's mark / count / scan / index kernels group the live rows of the listed landmarks by landmark; then ONE
// workgroup per map runs the whole minimisation (trust_region_minimizer.cc as oracle/ov2_oracle_ba.c restates it, the loop of
// pg_minimize_kernel).  Every pose is constant, so J'J is block diagonal: a point keeps its 3 x 3 block and its gradient, and
// the model cost change -m.(r + m/2), m = J step, is -(step.g + step'Hstep / 2) -- no row is needed again once its point
// has been evaluated, and a candidate is evaluated WITH its block so that an accepted step costs one pass over the rows.
// A point belongs to a 16-lane quarter of a wave (3-80 rows: a dozen on average), rows strided over the lanes in keyframe
// order, sums by the fixed butterfly of ov2_wave.h; quarter q takes the points q, q + 16, ... of the list of entered points, in
// that order, and its running sums meet the other quarters' in a fixed tree.  What a point needs between passes (x, candidate,
// scale, LM diagonal, two blocks and gradients) lives in SP_N doubles of the map's solver block and is only ever touched by
// its own quarter; a row is re-evaluated from the tables every pass (pose -> R, projection, corrector): f64 arithmetic is not
// what bounds a single workgroup, the dependent loads row -> keyframe -> pose are.  The sorted rows of a point go to obs_off:
// the call ends what the last set-up can be updated from, so that array is free until the next set-up writes it.
#define SB_THREADS 256
#define SB_SUB 16
#define SB_GROUPS (SB_THREADS / SB_SUB)
enum { SP_X = 0, SP_CAND = 3, SP_SCALE = 6, SP_DIAG = 9, SP_H = 12 /* 2 x 6: upper triangles */, SP_G = 24 /* 2 x 3 */, SP_N = 30 };

struct sb_cam { double Kl[4], Kr[4], Rrl[9], trl[3]; };
struct sb_opt {
    double huber_a, ftol, initial_radius, max_radius, min_radius, min_d, max_d, min_rel, ptol, gtol;
    int max_iters, jacobi, max_invalid;
};

// ordered sum of one double per thread, total to every thread: the wave tree of ov2_wave.h, then the four waves as (0 + 1) + (2 + 3)
__device__ __forceinline__ double sb_block_sum(double v, double *sh4)
{
    v = ov2wave::wave_sum_f64(v);
    __syncthreads();   // the readers of the last sum are done with sh4
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

__device__ __forceinline__ double sb_block_max(double v, double *sh4)
{
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(sh4[0], sh4[1]), fmax(sh4[2], sh4[3]));
}

// One residual block of an XYZ point: what eval_row / huber / the corrector of ba.hip compute for OV2_BA_L_XYZ and
// OV2_BA_R_XYZ (src/ceres_parametrization.cpp:107-298, corrector.cc:42-157), restated for a constant pose.  Mr maps world
// directions into the measuring camera, cam is the point there.  Adds the block's cost, J'J (upper triangle) and J'r.
__device__ __forceinline__ void sb_block(const double *K, const double *Mr, const double *cam, double u, double v, double inv_sigma,
                                         double huber_a, double &cost, double *H, double *g)
{
    const double invz = 1.0 / cam[2];
    double r0 = inv_sigma * ((K[0] * cam[0] * invz + K[2]) - u);
    double r1 = inv_sigma * ((K[1] * cam[1] * invz + K[3]) - v);
    const double chi2 = r0 * r0 + r1 * r1;
    const bool use_loss = huber_a > 0.0;
    double rho0 = chi2, rho1 = 1.0, rho2 = 0.0;
    if (use_loss) {
        const double b = huber_a * huber_a;
        if (chi2 > b) {
            const double r = sqrt(chi2);
            rho0 = 2.0 * huber_a * r - b;
            rho1 = fmax(2.2250738585072014e-308, huber_a / r);
            rho2 = -rho1 / (2.0 * chi2);
        }
    }
    cost += 0.5 * rho0;
    const double invz2 = invz * invz;
    const double a0 = invz * K[0], a2 = -cam[0] * invz2 * K[0], b1 = invz * K[1], b2 = -cam[1] * invz2 * K[1];
    double Ja[3], Jb[3];   // the two rows of d r / d X = J_proj * Mr / sigma
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Ja[c] = inv_sigma * (a0 * Mr[c] + 0.0 * Mr[3 + c] + a2 * Mr[6 + c]);
        Jb[c] = inv_sigma * (0.0 * Mr[c] + b1 * Mr[3 + c] + b2 * Mr[6 + c]);
    }
    if (use_loss) {
        const double sqrt_rho1 = sqrt(rho1);
        double rs = sqrt_rho1, asn = 0.0;
        if (!(chi2 == 0.0 || rho2 <= 0.0)) {   // never for Huber (rho'' <= 0): kept as the corrector states it
            const double D = 1.0 + 2.0 * chi2 * rho2 / rho1;
            const double alpha = 1.0 - sqrt(D);
            rs = sqrt_rho1 / (1 - alpha);
            asn = alpha / chi2;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (asn == 0.0) { Ja[c] *= sqrt_rho1; Jb[c] *= sqrt_rho1; }
            else {
                const double rtj = Ja[c] * r0 + Jb[c] * r1;
                Ja[c] = sqrt_rho1 * (Ja[c] - asn * r0 * rtj);
                Jb[c] = sqrt_rho1 * (Jb[c] - asn * r1 * rtj);
            }
        }
        r0 *= rs; r1 *= rs;
    }
    H[0] += Ja[0] * Ja[0] + Jb[0] * Jb[0]; H[1] += Ja[0] * Ja[1] + Jb[0] * Jb[1]; H[2] += Ja[0] * Ja[2] + Jb[0] * Jb[2];
    H[3] += Ja[1] * Ja[1] + Jb[1] * Jb[1]; H[4] += Ja[1] * Ja[2] + Jb[1] * Jb[2]; H[5] += Ja[2] * Ja[2] + Jb[2] * Jb[2];
    g[0] += Ja[0] * r0 + Jb[0] * r1; g[1] += Ja[1] * r0 + Jb[1] * r1; g[2] += Ja[2] * r0 + Jb[2] * r1;
}

// cost, J'J and J'r of one point at X over its `cnt` rows (sorted by keyframe): lane sl of the quarter takes the rows sl,
// sl + 16, ... in that order, left block before right block; the totals reach every lane of the quarter
__device__ __forceinline__ void sb_eval_point(const map_view &M, const sb_cam &C, double huber_a, const int *rows, int cnt, const double *X,
                                              int sl, double &cost, double *H, double *g)
{
    cost = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) H[i] = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    for (int t = sl; t < cnt; t += SB_SUB) {
        const int r = rows[t];
        const int flag = M.obs_flag[r];
        const double inv_sigma = 1.0 / (double)(1 << M.obs_scale[r]);   // sqrt_info = I / 2^scale
        double Rwc[9], twc[3], lcam[3], Mr[9];
        ov2se3::pose_Rt(M.kf_pose + 7 * (size_t)M.obs_kf[r], Rwc, twc);
        const double dd[3] = {X[0] - twc[0], X[1] - twc[1], X[2] - twc[2]};
#pragma unroll
        for (int q = 0; q < 3; ++q) lcam[q] = Rwc[q] * dd[0] + Rwc[3 + q] * dd[1] + Rwc[6 + q] * dd[2];   // Tcw * X
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) Mr[3 * q + c] = Rwc[3 * c + q];
        sb_block(C.Kl, Mr, lcam, M.obs_uv[2 * (size_t)r], M.obs_uv[2 * (size_t)r + 1], inv_sigma, huber_a, cost, H, g);
        if (flag & OBS_STEREO) {
            double rcam[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) rcam[q] = (C.Rrl[3 * q] * lcam[0] + C.Rrl[3 * q + 1] * lcam[1] + C.Rrl[3 * q + 2] * lcam[2]) + C.trl[q];
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) s += C.Rrl[3 * q + k] * Rwc[3 * c + k];
                    Mr[3 * q + c] = s;
                }
            sb_block(C.Kr, Mr, rcam, M.obs_ruv[2 * (size_t)r], M.obs_ruv[2 * (size_t)r + 1], inv_sigma, huber_a, cost, H, g);
        }
    }
    cost = ov2wave::row_sum_f64<SB_SUB>(cost);
#pragma unroll
    for (int i = 0; i < 6; ++i) H[i] = ov2wave::row_sum_f64<SB_SUB>(H[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = ov2wave::row_sum_f64<SB_SUB>(g[i]);
}

__device__ __forceinline__ void sb_logit(ov2_map_sba *R, int &n_log, double cost, double change, double radius, double rel, double model,
                                         int valid, int ok)
{
    if (n_log >= OV2_BA_MAX_LOG) return;
    if (threadIdx.x == 0) {
        ov2_ba_iter *it = &R->log[n_log];
        it->cost = cost; it->cost_change = change; it->radius = radius; it->relative_decrease = rel;
        it->model_cost_change = model; it->step_is_valid = valid; it->step_is_successful = ok;
    }
    ++n_log;
}

// Every thread carries the scalar state of the minimiser redundantly (all sums are broadcast), so the control flow is
// uniform over the workgroup; a quarter's loop over its points has a trip count of its own, and every barrier stands outside.
__global__ __launch_bounds__(SB_THREADS) void sb_solve_kernel(const map_job *__restrict__ J, sb_opt o)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, sl = tid & (SB_SUB - 1), grp = tid / SB_SUB;
    __shared__ sb_cam C;
    __shared__ double sh4[4];
    __shared__ int s_ent[SB_THREADS / 64], s_cnt[SB_THREADS / 64];
    ov2_map_sba *R = reinterpret_cast<ov2_map_sba *>(j.hdr_out);
    {   // the record starts as zeros: thread 0 alone writes it from here on, behind the barriers below
        int *Rw = reinterpret_cast<int *>(R);
        for (int k = tid; k < (int)(sizeof(ov2_map_sba) / sizeof(int)); k += SB_THREADS) Rw[k] = 0;
    }
    if (tid == 0 && j.mg_seg) {
        const double *c = j.sb_cam;   // ov2_map_sba_cam: calib_l | calib_r | T_rl
        for (int k = 0; k < 4; ++k) { C.Kl[k] = c[k]; C.Kr[k] = c[4 + k]; }
        ov2se3::pose_Rt(c + 8, C.Rrl, C.trl);
    }
    __syncthreads();
    if (!j.mg_seg) {   // uniform: an empty list leaves the map alone
        if (tid == 0) R->termination = OV2_BA_TERM_SKIPPED;
        return;
    }
    // ---- selection: the entries that count, and of them the points that enter, numbered in list order ----
    const int np = mg_npairs(j);
    int n_listed = 0, n_lm = 0;
    for (int base = 0; base < np; base += SB_THREADS) {
        const int i = base + tid;
        const bool counted = i < np && (!j.sb_status || j.sb_status[i] == OV2_MERGE_DONE);
        const int l = counted ? j.mg_new[i] : -1;
        bool enter = false;
        if ((unsigned)l < (unsigned)M.max_lm) {
            const int st = M.lm_state[l];
            enter = (st & OV2_LM_ALIVE) && (st & OV2_LM_3D) && j.mg_cnt[l] > 0 && j.mg_next[l] == ANCH_TOP - i;
        }
        const unsigned long long be = __ballot(enter), bc = __ballot(counted);
        if (lane == 0) { s_ent[wv] = __popcll(be); s_cnt[wv] = __popcll(bc); }
        __syncthreads();
        int before = n_lm;
        for (int w = 0; w < SB_THREADS / 64; ++w) {
            if (w < wv) before += s_ent[w];
            n_lm += s_ent[w]; n_listed += s_cnt[w];
        }
        // n_lm <= entries of the segment <= the entries the block was sized for
        if (enter) st_int(j.sb_lm + before + __popcll(be & ((1ull << lane) - 1ull)), l);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // ---- a point's rows in keyframe order (ranked as gt_fill_kernel ranks them), its block count, its start ----
    int nres = 0;
    for (int k = grp; k < n_lm; k += SB_GROUPS) {
        const int l = ld_int(j.sb_lm + k);
        const int cnt = j.mg_cnt[l];
        const int *rows = j.mg_rows + j.mg_start[l];
        int *srt = j.obs_off + j.mg_start[l];   // mg_start[l] + cnt <= GH_ROWS <= n_obs: inside the array
        for (int t0 = 0; t0 < cnt; t0 += SB_SUB) {
            const int t = t0 + sl;
            const bool on = t < cnt;
            const int r = on ? rows[t] : 0;
            const int kf = on ? M.obs_kf[r] : 0x7fffffff;
            int rank = 0;
            for (int u0 = 0; u0 < cnt; u0 += SB_SUB) {
                const int v = u0 + sl < cnt ? M.obs_kf[rows[u0 + sl]] : 0x7fffffff;
#pragma unroll
                for (int s = 0; s < SB_SUB; ++s) {
                    const int kv = __shfl(v, s, SB_SUB);
                    rank += (kv < kf || (kv == kf && u0 + s < t)) ? 1 : 0;
                }
            }
            if (on) {
                srt[rank] = r;
                nres += (M.obs_flag[r] & OBS_STEREO) ? 2 : 1;
            }
        }
        if (sl < 3) j.sb_pt[(size_t)k * SP_N + SP_X + sl] = M.lm_xyz[3 * (size_t)l + sl];
    }
    for (int s = 32; s; s >>= 1) nres += __shfl_xor(nres, s);
    if (lane == 0) s_ent[wv] = nres;
    __threadfence_block();
    __syncthreads();
    nres = 0;
    for (int w = 0; w < SB_THREADS / 64; ++w) nres += s_ent[w];
    if (tid == 0) { R->n_listed = n_listed; R->n_lm = n_lm; R->n_skipped = n_listed - n_lm; R->n_res = nres; }
    if (nres == 0) {   // uniform
        if (tid == 0) R->termination = OV2_BA_TERM_SKIPPED;
        return;
    }
    // ---- iteration zero: cost, blocks and gradients at x, the Jacobi scale, the gradient's max norm ----
    int cur = 0;   // which of a point's two (block, gradient) slots belongs to x; the other takes the candidate's
    double x_cost, gmax;
    {
        double cs = 0.0, gm = 0.0;
        for (int k = grp; k < n_lm; k += SB_GROUPS) {
            const int l = j.sb_lm[k];
            double *P = j.sb_pt + (size_t)k * SP_N;
            const double X[3] = {P[SP_X], P[SP_X + 1], P[SP_X + 2]};
            double c, H[6], g[3];
            sb_eval_point(M, C, o.huber_a, j.obs_off + j.mg_start[l], j.mg_cnt[l], X, sl, c, H, g);
            cs += c;
            // gradient_max_norm = || x - Plus(x, -g) ||_inf with the gradient of the unscaled problem
#pragma unroll
            for (int q = 0; q < 3; ++q) gm = fmax(gm, fabs(X[q] - (X[q] + (-g[q]))));
            if (sl == 0) {
#pragma unroll
                for (int q = 0; q < 6; ++q) P[SP_H + q] = H[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) P[SP_G + q] = g[q];
                P[SP_SCALE] = o.jacobi ? 1.0 / (1.0 + sqrt(H[0])) : 1.0;
                P[SP_SCALE + 1] = o.jacobi ? 1.0 / (1.0 + sqrt(H[3])) : 1.0;
                P[SP_SCALE + 2] = o.jacobi ? 1.0 / (1.0 + sqrt(H[5])) : 1.0;
            }
        }
        x_cost = sb_block_sum(sl == 0 ? cs : 0.0, sh4);
        gmax = sb_block_max(gm, sh4);
    }
    const double initial_cost = x_cost;
    double x_norm = -1.0, radius = o.initial_radius, decrease_factor = 2.0;
    int reuse_diagonal = 0, invalid_steps = 0, iteration = 0, last_ok = 1, term = OV2_BA_TERM_MAX_ITER, n_log = 0;
    sb_logit(R, n_log, x_cost, 0.0, radius, 0.0, 0.0, 1, 1);
    for (;;) {
        if (iteration >= o.max_iters) { term = OV2_BA_TERM_MAX_ITER; break; }
        if (last_ok && gmax <= o.gtol) { term = OV2_BA_TERM_GTOL; break; }
        if (radius <= o.min_radius) { term = OV2_BA_TERM_MIN_RADIUS; break; }
        ++iteration;
        // LevenbergMarquardtStrategy::ComputeStep per point: (H + D'D) y = g on the scaled block, step = -y, candidate = x + scale * step
        double mc = 0.0, sn = 0.0;
        int bad = 0;
        for (int k = grp; k < n_lm; k += SB_GROUPS) {
            double *P = j.sb_pt + (size_t)k * SP_N;
            const double *Hu = P + SP_H + 6 * cur, *gu = P + SP_G + 3 * cur;
            const double s0 = P[SP_SCALE], s1 = P[SP_SCALE + 1], s2 = P[SP_SCALE + 2];
            const double h00 = Hu[0] * s0 * s0, h01 = Hu[1] * s0 * s1, h02 = Hu[2] * s0 * s2, h11 = Hu[3] * s1 * s1, h12 = Hu[4] * s1 * s2,
                         h22 = Hu[5] * s2 * s2;
            const double g0 = gu[0] * s0, g1 = gu[1] * s1, g2 = gu[2] * s2;
            double d0, d1, d2;
            if (!reuse_diagonal) {
                d0 = fmin(fmax(h00, o.min_d), o.max_d); d1 = fmin(fmax(h11, o.min_d), o.max_d); d2 = fmin(fmax(h22, o.min_d), o.max_d);
                if (sl == 0) { P[SP_DIAG] = d0; P[SP_DIAG + 1] = d1; P[SP_DIAG + 2] = d2; }
            } else { d0 = P[SP_DIAG]; d1 = P[SP_DIAG + 1]; d2 = P[SP_DIAG + 2]; }
            const double l0 = sqrt(d0 / radius), l1 = sqrt(d1 / radius), l2 = sqrt(d2 / radius);
            // lower Cholesky of the 3 x 3 block and the two triangular solves, in the oracle's order
            const double a00 = l0 * l0 + h00, a11 = l1 * l1 + h11, a22 = l2 * l2 + h22;
            bool ok = a00 > 0.0;
            const double c00 = sqrt(a00), c10 = h01 / c00, c20 = h02 / c00;
            const double e1 = a11 - c10 * c10;
            ok = ok && e1 > 0.0;
            const double c11 = sqrt(e1), c21 = (h12 - c20 * c10) / c11;
            const double e2 = (a22 - c20 * c20) - c21 * c21;
            ok = ok && e2 > 0.0;
            const double c22 = sqrt(e2);
            const double z0 = g0 / c00, z1 = (g1 - c10 * z0) / c11, z2 = ((g2 - c20 * z0) - c21 * z1) / c22;
            const double y2 = z2 / c22, y1 = (z1 - c21 * y2) / c11, y0 = ((z0 - c10 * y1) - c20 * y2) / c00;
            const double t0 = -y0, t1 = -y1, t2 = -y2;
            if (!ok || !isfinite(t0) || !isfinite(t1) || !isfinite(t2)) { bad = 1; continue; }
            // model_cost_change = -m.(r + m / 2), m = J step, summed over the point's rows: -(step.g + step'H step / 2)
            const double Hs0 = h00 * t0 + h01 * t1 + h02 * t2, Hs1 = h01 * t0 + h11 * t1 + h12 * t2, Hs2 = h02 * t0 + h12 * t1 + h22 * t2;
            mc -= (t0 * g0 + t1 * g1 + t2 * g2) + 0.5 * (t0 * Hs0 + t1 * Hs1 + t2 * Hs2);
            const double x0 = P[SP_X], x1 = P[SP_X + 1], x2 = P[SP_X + 2];
            const double q0 = x0 + t0 * s0, q1 = x1 + t1 * s1, q2 = x2 + t2 * s2;
            sn += (x0 - q0) * (x0 - q0) + (x1 - q1) * (x1 - q1) + (x2 - q2) * (x2 - q2);
            if (sl == 0) { P[SP_CAND] = q0; P[SP_CAND + 1] = q1; P[SP_CAND + 2] = q2; }
        }
        reuse_diagonal = 1;
        const bool finite = !__syncthreads_or(bad);
        double model_change = 0.0;
        bool valid = false;
        if (finite) {
            model_change = sb_block_sum(sl == 0 ? mc : 0.0, sh4);
            valid = model_change > 0.0;
        }
        if (!valid) {   // HandleInvalidStep
            if (++invalid_steps >= o.max_invalid) { term = OV2_BA_TERM_FAILURE; break; }
            radius = radius / decrease_factor; decrease_factor *= 2.0;
            last_ok = 0;
            sb_logit(R, n_log, x_cost, 0.0, radius, 0.0, model_change, 0, 0);
            continue;
        }
        invalid_steps = 0;
        const double step_norm = sqrt(sb_block_sum(sl == 0 ? sn : 0.0, sh4));
        // the candidate: its cost, and its blocks and gradients into the points' other slots
        double cs = 0.0, gm = 0.0, xs = 0.0;
        for (int k = grp; k < n_lm; k += SB_GROUPS) {
            const int l = j.sb_lm[k];
            double *P = j.sb_pt + (size_t)k * SP_N;
            const double X[3] = {P[SP_CAND], P[SP_CAND + 1], P[SP_CAND + 2]};
            double c, H[6], g[3];
            sb_eval_point(M, C, o.huber_a, j.obs_off + j.mg_start[l], j.mg_cnt[l], X, sl, c, H, g);
            cs += c;
            xs += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
#pragma unroll
            for (int q = 0; q < 3; ++q) gm = fmax(gm, fabs(X[q] - (X[q] + (-g[q]))));
            if (sl == 0) {
#pragma unroll
                for (int q = 0; q < 6; ++q) P[SP_H + 6 * (cur ^ 1) + q] = H[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) P[SP_G + 3 * (cur ^ 1) + q] = g[q];
            }
        }
        const double cand_cost = sb_block_sum(sl == 0 ? cs : 0.0, sh4);
        if (step_norm <= o.ptol * (x_norm + o.ptol)) { term = OV2_BA_TERM_PTOL; break; }
        const double cost_change = x_cost - cand_cost;
        if (fabs(cost_change) <= o.ftol * x_cost) {   // FunctionToleranceReached: returns WITHOUT taking the candidate
            term = OV2_BA_TERM_FTOL;
            sb_logit(R, n_log, x_cost, cost_change, radius, 0.0, model_change, 1, 0);
            break;
        }
        const double rel = (cand_cost >= 1.7976931348623157e308) ? -1.7976931348623157e308 : (x_cost - cand_cost) / model_change;
        if (rel > o.min_rel) {   // HandleSuccessfulStep: x <- candidate, whose evaluation stands in the other slots
            for (int k = grp; k < n_lm; k += SB_GROUPS) {
                double *P = j.sb_pt + (size_t)k * SP_N;
                if (sl < 3) P[SP_X + sl] = P[SP_CAND + sl];
            }
            cur ^= 1;
            x_norm = sqrt(sb_block_sum(sl == 0 ? xs : 0.0, sh4));
            x_cost = cand_cost;
            gmax = sb_block_max(gm, sh4);
            radius = fmin(o.max_radius, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3)));   // StepAccepted
            decrease_factor = 2.0;
            reuse_diagonal = 0;
            last_ok = 1;
            sb_logit(R, n_log, x_cost, cost_change, radius, rel, model_change, 1, 1);
        } else {                 // StepRejected
            radius = radius / decrease_factor; decrease_factor *= 2.0;
            last_ok = 0;
            sb_logit(R, n_log, cand_cost, cost_change, radius, rel, model_change, 1, 0);
        }
    }
    // the minimiser's final state: the last accepted x (an accepted step lowered the cost, so it is the best one too)
    for (int k = grp; k < n_lm; k += SB_GROUPS) {
        const int l = j.sb_lm[k];
        if (sl < 3) j.lm_xyz_w[3 * (size_t)l + sl] = j.sb_pt[(size_t)k * SP_N + SP_X + sl];
    }
    if (tid == 0) { R->termination = term; R->n_log = n_log; R->initial_cost = initial_cost; R->final_cost = x_cost; }
}

// ---- match gather: the flat input of Mapper::matchToMap (src/mapper.cpp:576-774) from the tables -------------------------------
// The merge stage's mark / count / scan / index kernels group the live rows of the landmarks a call names -- here the
// landmarks of the new keyframe's keypoints and of the candidates -- by landmark (mg_start / mg_cnt / mg_rows).  One entry
// (keypoint or candidate) then belongs to a 16-lane quarter of a wave: a landmark has a row per observing keyframe, a dozen
// on average, so a whole wave per entry would idle three quarters of its lanes.  The counting pass leaves the entry's
// observer and descriptor counts where the prefix offsets go, a flat in-place scan over the WHOLE batch turns them into the
// contiguous *_ptr arrays the matcher reads across frame boundaries, and the filling pass ranks the entry's rows by kfid
// (MapPoint::set_kfids_ is a std::set: ascending; table order is not keyframe order once rows were appended late or
// relabelled) and copies.  No LDS: the ranks come from 16-lane shuffles, the descriptors move as 16-byte halves, lane h of
// the quarter taking half h of the chunk so that the quarter's stores are one contiguous run.
#define GT_SUB 16

// the quarter's 16 bits of a wave-wide vote
__device__ __forceinline__ unsigned gt_vote(bool p) { return (unsigned)((__ballot(p) >> (threadIdx.x & 48)) & 0xffffull); }

struct gt_entry { bool is_kp; int flat, lm, state, cnt; const int *rows; };

// entry e of map j: its landmark, the landmark's state (0 = out of range) and its live rows (none for a dead landmark)
__device__ __forceinline__ gt_entry gt_entry_of(const map_job &j, int e)
{
    gt_entry E;
    E.is_kp = e < j.gt_nkp;
    E.flat = E.is_kp ? j.gt_kp0 + e : j.gt_cand0 + (e - j.gt_nkp);
    E.lm = E.is_kp ? j.gt_kp_lmid[e] : j.gt_cand_lmid[e - j.gt_nkp];
    const bool inr = (unsigned)E.lm < (unsigned)j.M.max_lm;
    E.state = inr ? j.M.lm_state[E.lm] : 0;
    const bool alive = E.state & OV2_LM_ALIVE;
    E.cnt = alive ? j.mg_cnt[E.lm] : 0;
    E.rows = j.mg_rows + (alive ? j.mg_start[E.lm] : 0);
    return E;
}

__global__ __launch_bounds__(256) void gt_count_kernel(const map_job *__restrict__ J, gather_out G)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int tid = threadIdx.x, sl = tid & (GT_SUB - 1);
    // the map's pose table behind those of the maps before it (kfid indexes it), and the pose the candidates are projected with
    for (size_t t = (size_t)blockIdx.x * 256 + tid; t < 7 * (size_t)M.max_kf; t += (size_t)gridDim.x * 256)
        G.kf_Twc[7 * (size_t)j.gt_kf0 + t] = M.kf_pose[t];
    if (blockIdx.x == 0 && tid < 7) G.Twc[7 * blockIdx.y + tid] = M.kf_pose[7 * (size_t)j.newkf + tid];
    const int e = (blockIdx.x * 256 + tid) / GT_SUB;
    if (e >= j.gt_nkp + j.gt_ncand) return;   // uniform per quarter
    const gt_entry E = gt_entry_of(j, e);
    int nd = 0; unsigned in_new = 0;
    for (int t0 = 0; t0 < E.cnt; t0 += GT_SUB) {   // the trip count is uniform per quarter
        const bool on = t0 + sl < E.cnt;
        const int r = on ? E.rows[t0 + sl] : 0;
        nd += __popc(gt_vote(on && M.obs_hasdesc[r]));
        in_new |= gt_vote(on && M.obs_kf[r] == j.newkf);
    }
    // keypoint: map point present with descriptors (src/mapper.cpp:676-685); candidate: alive, 3-D, not observed by the new
    // keyframe, with descriptors (:613-624).  Everything else gets two empty ranges.
    const bool ok = nd > 0 && (E.is_kp || ((E.state & OV2_LM_3D) && !in_new));
    if (sl == 0) {
        (E.is_kp ? G.kp_kf_ptr : G.cand_kf_ptr)[E.flat] = ok ? E.cnt : 0;
        (E.is_kp ? G.kp_desc_ptr : G.cand_desc_ptr)[E.flat] = ok ? nd : 0;
    }
}

__global__ __launch_bounds__(256) void gt_fill_kernel(const map_job *__restrict__ J, gather_out G)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int tid = threadIdx.x, sl = tid & (GT_SUB - 1);
    const int e = (blockIdx.x * 256 + tid) / GT_SUB;
    if (e >= j.gt_nkp + j.gt_ncand) return;   // uniform per quarter
    const gt_entry E = gt_entry_of(j, e);
    if (E.is_kp) {   // Keypoint::px_ of the new keyframe's own row; (0, 0) where the keyframe holds no live row of the landmark
        unsigned found = 0;
        for (int t0 = 0; t0 < E.cnt; t0 += GT_SUB) {
            const bool on = t0 + sl < E.cnt;
            const int r = on ? E.rows[t0 + sl] : 0;
            const bool hit = on && M.obs_kf[r] == j.newkf;
            if (hit) G.kp_px[E.flat] = M.obs_px[r];
            found |= gt_vote(hit);
        }
        if (!found && sl == 0) G.kp_px[E.flat] = make_float2(0.f, 0.f);
    } else if (sl < 3) {
        G.cand_wpt[3 * (size_t)E.flat + sl] = (E.state & OV2_LM_ALIVE) ? M.lm_xyz[3 * (size_t)E.lm + sl] : 0.0;
    }
    const int *kf_ptr = E.is_kp ? G.kp_kf_ptr : G.cand_kf_ptr, *desc_ptr = E.is_kp ? G.kp_desc_ptr : G.cand_desc_ptr;
    const int k0 = kf_ptr[E.flat], kn = kf_ptr[E.flat + 1] - k0, d0 = desc_ptr[E.flat];
    // an accepted entry lists all its live rows (kn == cnt); distinct landmarks per list keep the total within the tables' rows
    if (kn <= 0 || kn != E.cnt || k0 + kn > G.cap_rows) return;
    int *kfids = E.is_kp ? G.kp_kfids : G.cand_kfids;
    uint4 *descs = E.is_kp ? G.kp_descs : G.cand_descs;
    int dbase = 0;
    for (int t0 = 0; t0 < E.cnt; t0 += GT_SUB) {
        const int t = t0 + sl;
        const bool on = t < E.cnt;
        const int r = on ? E.rows[t] : 0;
        const int kf = on ? M.obs_kf[r] : 0x7fffffff;
        int rank = 0;   // rows of the landmark with a smaller keyframe (equal ones, which one landmark never has, by their place)
        for (int u0 = 0; u0 < E.cnt; u0 += GT_SUB) {
            const int v = u0 + sl < E.cnt ? M.obs_kf[E.rows[u0 + sl]] : 0x7fffffff;
#pragma unroll
            for (int s = 0; s < GT_SUB; ++s) {
                const int kv = __shfl(v, s, GT_SUB);
                rank += (kv < kf || (kv == kf && u0 + s < t)) ? 1 : 0;
            }
        }
        if (on) {
            kfids[k0 + rank] = kf;
            if (E.is_kp) G.kp_kf_px[k0 + rank] = M.obs_px[r];
        }
        // the described rows of the chunk, 32 bytes each: half h of the chunk's run goes through lane h (and h + 16)
        const unsigned mask = gt_vote(on && M.obs_hasdesc[r]);
        const int nh = 2 * __popc(mask);
#pragma unroll
        for (int h0 = 0; h0 < 2 * GT_SUB; h0 += GT_SUB) {
            const int h = h0 + sl, q = h >> 1;
            unsigned mm = mask;
            for (int i = 0; i < q && mm; ++i) mm &= mm - 1;   // drop the q lowest described lanes
            const int src = mm ? __ffs(mm) - 1 : 0;
            const int rr = __shfl(r, src, GT_SUB);
            if (h < nh) descs[2 * (size_t)(d0 + dbase + q) + (h & 1)] = M.obs_desc[2 * (size_t)rr + (h & 1)];
        }
        dbase += nh >> 1;
    }
}

// ---- update stage of Optimizer::localPoseGraph (src/optimizer.cpp:2476-2577) on the tables ------------------------------
// The free keyframes of the graph (listed, ascending, last = newkf) take their optimised poses, every younger keyframe k
// moves rigidly with the new one (opt * (ini * old(k)), ini = inverse(old(newkf))), and a landmark moves with the keyframe
// that anchors it (MapPoint::kfid_ = its oldest live observer) when that keyframe moved and the landmark's keypoints are
// 3D: xyz' = new(a) * (inverse(old(a)) * xyz).  Three scans: anchors (rows), landmarks -- which read the OLD poses and
// work out new(a) themselves --, then the poses.  ini and T_corr = opt * ini are written once, by the first scan, into
// the map's slot behind its gathered header, so that no scan reads the pose of newkf while another lane replaces it.
enum { PH_KF_CHAIN = 0, PH_KF_YOUNGER, PH_LM_MOVED };

// SE3::operator*(Vec3) of the host mirror
__device__ __forceinline__ void se3_apply(const double *T, const double *p, double out[3])
{
    double R[9];
    ov2se3::pose_R(T, R);
    out[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + T[0];
    out[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + T[1];
    out[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + T[2];
}

// the device-side gate of a map (ov2_map_pose_graph_update_batch_dev, ov2_map_local_pose_graph_batch); uniform per map
__device__ __forceinline__ bool pg_skipped(const map_job &j) { return j.pg_skip && *j.pg_skip; }

// ---- Optimizer::assembleLocalPoseGraph (src/optimizer.cpp:2361-2425) from the pose table --------------------------------
// The host derived the chain (loop keyframe after the walk-up, then the live keyframes up to newkf) from its copy of the
// keyframe states; only the values come from the device.  Lane i copies pose i of the chain and writes the edge that ENDS
// in it: T_ij = Tciw * Twcj with Tciw = inverse(pose i - 1) (:2400-2415), in the host mirror's SE3 arithmetic; lane 0
// writes the closing edge (0, lp_n - 1), inverse(Twc_loop) * newTwc (:2387, :2422-2425), behind the lp_n - 1 odometry
// edges.  Every lane reads the table and writes its own seven + seven doubles: nothing is shared, nothing is reduced, and
// the launch is bounded by the latency of two dependent loads per lane (the id, then the poses).
__global__ __launch_bounds__(256) void mp_assemble_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j.lp_n) return;
    const double *Tj = j.M.kf_pose + 7 * (size_t)j.lp_kfid[i];
    double Tciw[7], T[7];
    if (i == 0) {
        se3_inverse(Tj, Tciw);
        se3_mul(Tciw, j.lp_newTwc, T);
    } else {
        se3_inverse(j.M.kf_pose + 7 * (size_t)j.lp_kfid[i - 1], Tciw);
        se3_mul(Tciw, Tj, T);
    }
    double *e = j.lp_Tij + 7 * (size_t)(i == 0 ? j.lp_n - 1 : i - 1);
#pragma unroll
    for (int q = 0; q < 7; ++q) { j.lp_pose[7 * (size_t)i + q] = Tj[q]; e[q] = T[q]; }
}

// the degenerate-solution test of Optimizer::applyLocalPoseGraph (:2468-2474) on the solved block, one lane per map:
// stereo && |t(newTwc) - t(optimised pose of newkf)| > 0.3, the f64 expression of the host stage.  The lane leaves the
// map's skip byte for the update kernels, its verdict behind the gathered header and, for a map that is not DONE, a zero
// in its slot of the caller's pair counts.
__global__ __launch_bounds__(64) void mp_gate_kernel(const map_job *__restrict__ J, int B)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const map_job &j = J[b];
    int verdict = OV2_LPG_NO_CHAIN;
    if (j.lp_n) {
        const double *opt = j.lp_pose + 7 * (size_t)(j.lp_n - 1), *nw = j.lp_newTwc;
        const double dx = nw[0] - opt[0], dy = nw[1] - opt[1], dz = nw[2] - opt[2];
        const bool deg = __dsqrt_rn(dx * dx + dy * dy + dz * dz) > 0.3 && j.lp_stereo;
        verdict = deg ? OV2_LPG_DEGENERATE : OV2_LPG_DONE;
        *j.lp_skip = deg ? 1 : 0;
    }
    *j.lp_verdict = verdict;
    if (j.lp_npairs && verdict != OV2_LPG_DONE) *j.lp_npairs = 0;
}

// place of keyframe kf in the ascending list, -1 when it is not listed
__device__ __forceinline__ int pg_listed(const map_job &j, int kf)
{
    int lo = 0, hi = j.pg_n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, v = j.pg_kfid[mid];
        if (v == kf) return mid;
        if (v < kf) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// the pose keyframe k ends with: its listed pose, opt * (ini * old(k)) when it is younger than newkf, else none (false).
// For a keyframe that moves both candidates are formed and one is selected element by element: nothing is indexed
// dynamically, nothing spills.
__device__ __forceinline__ bool pg_new_pose(const map_job &j, int k, double out[7], bool &listed)
{
    const int idx = pg_listed(j, k);
    listed = idx >= 0;
    if (!listed && k <= j.newkf) return false;      // neither listed nor younger: nothing to work out
    double rel[7], y[7];
    se3_mul(j.pg_tmp, j.M.kf_pose + 7 * (size_t)k, rel);
    se3_mul(j.pg_Twc + 7 * (size_t)(j.pg_n - 1), rel, y);
    const double *L = j.pg_Twc + 7 * (size_t)(listed ? idx : 0);
#pragma unroll
    for (int q = 0; q < 7; ++q) out[q] = listed ? L[q] : y[q];
    return true;
}

__global__ __launch_bounds__(256) void mp_anchor_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.pg_n) return;
    const bool skip = pg_skipped(j);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double ini[7], corr[7];
        se3_inverse(M.kf_pose + 7 * (size_t)j.newkf, ini);
        se3_mul(j.pg_Twc + 7 * (size_t)(j.pg_n - 1), ini, corr);
#pragma unroll
        for (int q = 0; q < 7; ++q) { j.pg_tmp[q] = skip ? 0.0 : ini[q]; j.pg_tmp[7 + q] = skip ? 0.0 : corr[q]; }
    }
    if (skip) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i >= M.n_obs || !obs_live(M, i, kf, lm)) return;
    atomicMax(&j.tt_old[lm], ANCH_TOP - kf);       // the smallest kfid wins
}

// one lane per landmark; the poses are still the old ones
__global__ __launch_bounds__(256) void mp_landmarks_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.pg_n || (int)blockIdx.x * 256 >= M.max_lm || pg_skipped(j)) return;   // uniform per workgroup
    const int l = blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (l < M.max_lm) {
        const unsigned char st = M.lm_state[l];
        const int o = j.tt_old[l];
        if ((st & OV2_LM_ALIVE) && (st & OV2_LM_KP3D) && o) {
            const int a = ANCH_TOP - o;
            double Tnew[7];
            bool listed;
            if (pg_new_pose(j, a, Tnew, listed)) {
                double Tcw[7], cam[3], w[3];
                se3_inverse(M.kf_pose + 7 * (size_t)a, Tcw);
                se3_apply(Tcw, M.lm_xyz + 3 * (size_t)l, cam);      // Frame::projWorldToCam
                se3_apply(Tnew, cam, w);
                j.lm_xyz_w[3 * (size_t)l] = w[0]; j.lm_xyz_w[3 * (size_t)l + 1] = w[1]; j.lm_xyz_w[3 * (size_t)l + 2] = w[2];
                j.lm_state_w[l] = st | OV2_LM_3D;                   // MapManager::updateMapPoint -> MapPoint::setPoint
                moved = true;
            }
        }
    }
    const unsigned long long bal = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&j.hdr[PH_LM_MOVED], __popcll(bal));
}

// one lane per keyframe: a lane reads its own old pose only (and ini from the map's slot)
__global__ __launch_bounds__(256) void mp_poses_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.pg_n || (int)blockIdx.x * 256 >= M.max_kf || pg_skipped(j)) return;   // uniform per workgroup
    const int k = blockIdx.x * 256 + threadIdx.x;
    bool listed = false, moved = false;
    if (k < M.max_kf && M.kf_state[k]) {
        double T[7];
        moved = pg_new_pose(j, k, T, listed);
        if (moved) {
#pragma unroll
            for (int q = 0; q < 7; ++q) j.kf_pose_w[7 * (size_t)k + q] = T[q];
        }
    }
    const unsigned long long bl = __ballot(moved && listed), by = __ballot(moved && !listed);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicAdd(&j.hdr[PH_KF_CHAIN], __popcll(bl));
        if (by) atomicAdd(&j.hdr[PH_KF_YOUNGER], __popcll(by));
    }
}

// ---- Optimizer::looseBA (src/optimizer.cpp:900-1672) on the tables ------------------------------------------------------
// Set-up (:985-1270): the chain of localBA's set-up with another keyframe selection.  The live keyframes of
// [lb_lo, newkf] in ascending id: the first nmin_cst are constant, the rest optimised (:1004-1030); no covisibility, no
// abort.  One wave per map, 64 keyframes per step; the constants handed out so far ride in a wave-uniform register.
__global__ __launch_bounds__(64) void ml_select_kernel(const map_job *__restrict__ J, int nmin_cst)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int lane = threadIdx.x, hi = min(j.newkf, M.max_kf - 1);
    int nlive = 0;
    for (int base = j.lb_lo; base <= hi; base += 64) {
        const int kf = base + lane;
        const bool live = kf <= hi && M.kf_state[kf];
        const unsigned long long bal = __ballot(live);
        const int rank = nlive + __popcll(bal & ((1ull << lane) - 1ull));   // live keyframes of the range before this one
        if (live) j.kf_role[kf] = rank < nmin_cst ? 2 : 1;
        nlive += __popcll(bal);
    }
    if (lane == 0) j.hdr[MH_NMAXKF] = j.newkf;   // observers younger than the loop keyframe are left out (:1056)
}

// Update (:1330-1657).  Counters of the stage, behind the map's gathered header (the set-up's header keeps MH_NRM_LM,
// MH_NRM_OBS and MH_NST_OFF, which mu_obs_kernel counts):
enum { LB_FLAG_L = 0, LB_FLAG_R, LB_WRITTEN, LB_PROP, LB_YOUNGER, LB_BAD, LB_FREE, LB_N = 8 };
enum { LB_EXTRA_INTS = LB_N + 42 };   // + 21 doubles: inverse(old(newkf)) | opt | T_corr

__device__ __forceinline__ void lb_count(const map_job &j, int which, bool hit)
{
    const unsigned long long bal = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&j.lb_cnt[which], __popcll(bal));
}

// launch 1, one lane per landmark: observer counts and oldest observers start from zero; one lane of the map's first
// workgroup works out the constants of the statement from the OLD pose of the loop keyframe and its solved one (:1432-1436)
__global__ __launch_bounds__(256) void ml_clear_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (blockIdx.x == 0 && (int)threadIdx.x < LB_N) j.lb_cnt[threadIdx.x] = 0;
    if (!j.lb_on) return;
    if (blockIdx.x == 0 && threadIdx.x == 64) {
        const flat_out O = flat_of(j, inv);
        const double *opt = O.pose + 7 * (size_t)j.kf_idx[j.newkf];
        double ini[7], corr[7];
        se3_inverse(M.kf_pose + 7 * (size_t)j.newkf, ini);
        se3_mul(opt, ini, corr);
#pragma unroll
        for (int q = 0; q < 7; ++q) { j.lb_tmp[q] = ini[q]; j.lb_tmp[7 + q] = opt[q]; j.lb_tmp[14 + q] = corr[q]; }
    }
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < M.max_lm) { j.lm_nobs[l] = 0; j.lm_pack[l] = 0ull; }
}

// launch 2, one lane per row of the table as it is now: observers and the oldest observer (MapPoint::kfid_, with its row
// for the anchor pixel) of EVERY landmark, before anything is removed; the rows of the set-up also count their flagged
// blocks by camera
__global__ __launch_bounds__(256) void ml_observers_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.lb_on || (int)blockIdx.x * 256 >= M.n_obs) return;   // uniform per workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    int kf, lm;
    if (i < M.n_obs && obs_live(M, i, kf, lm)) {
        atomicAdd(&j.lm_nobs[lm], 1);
        atomicMax(&j.lm_pack[lm], ((unsigned long long)(ANCH_TOP - kf) << 32) | (unsigned)i);
    }
    int nl = 0, nr = 0;
    if (j.outlier && i < j.last_n_obs) {
        const int c = j.obs_cnt[i];
        if (c) {
            const flat_out O = flat_of(j, inv);
            const int o = j.obs_off[i];
            for (int k = 0; k < c; ++k)
                if (j.outlier[o + k]) {
                    const int t = O.res_type[o + k];
                    if (t == OV2_BA_L_XYZ || t == OV2_BA_L_INV) ++nl; else ++nr;
                }
        }
    }
    // at most two blocks per row: two ballots count them
    lb_count(j, LB_FLAG_L, nl > 0);
    lb_count(j, LB_FLAG_R, nr > 0);
}

// launch 3, one lane per landmark, every pose still the OLD one.  A local landmark (:1440-1526): isBad() / non-positive
// depth / anchor outside the problem -> the bad set (bit 8 of lm_sel); otherwise its new point -- with inverse depth from
// the pose of its oldest observer BEFORE the update (:1499-1511) --, 3D with its keypoints (MapManager::updateMapPoint).
// Any other landmark whose keypoints are 3D and whose oldest observer is younger than the loop keyframe moves with that
// keyframe (:1571-1592): xyz' = (opt * (ini * old(a))) * (inverse(old(a)) * xyz).
__global__ __launch_bounds__(256) void ml_landmarks_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.lb_on || (int)blockIdx.x * 256 >= M.max_lm) return;   // uniform per workgroup
    const int l = blockIdx.x * 256 + threadIdx.x;
    bool written = false, moved = false;
    if (l < M.max_lm) {
        int st = M.lm_state[l];
        const unsigned long long oldest = j.lm_pack[l];   // 0: no live observer
        const int a = oldest ? ANCH_TOP - (int)(oldest >> 32) : -1;
        if ((st & OV2_LM_ALIVE) && j.lm_sel[l] == 1) {
            const int nobs = j.lm_nobs[l];
            const bool isobs = st & OV2_LM_OBS;
            bool bad = false;
            double w[3] = {0.0, 0.0, 0.0};
            if ((nobs < 2 && !isobs && (st & OV2_LM_3D)) || (nobs == 0 && !isobs)) {   // MapPoint::isBad clears is3d_
                bad = true;
                j.lm_state_w[l] = (unsigned char)(st & ~OV2_LM_3D);
            } else if (!j.lm_flag[l]) {
                bad = true;                                          // not in the problem (:1455)
            } else {
                const flat_out O = flat_of(j, inv);
                const int q = (int)(j.lm_pidx[l] & 0xffffffffull);
                if (inv) {
                    const double zanch = 1.0 / O.lm[q];
                    if (zanch <= 0.0 || a < 0 || j.kf_role[a] == 0) bad = true;   // :1470, :1478
                    else {
                        const int r = (int)(oldest & 0xffffffffull);
                        const double u = M.obs_uv[2 * (size_t)r], v = M.obs_uv[2 * (size_t)r + 1];
                        const double cam[3] = {zanch * (u - j.K[2]) / j.K[0], zanch * (v - j.K[3]) / j.K[1], zanch};
                        se3_apply(M.kf_pose + 7 * (size_t)a, cam, w);
                        written = true;
                    }
                } else {
                    w[0] = O.lm[3 * (size_t)q]; w[1] = O.lm[3 * (size_t)q + 1]; w[2] = O.lm[3 * (size_t)q + 2];
                    written = true;
                }
            }
            if (bad) atomicOr(&j.lm_sel[l], 8);
            if (written) {
                j.lm_xyz_w[3 * (size_t)l] = w[0]; j.lm_xyz_w[3 * (size_t)l + 1] = w[1]; j.lm_xyz_w[3 * (size_t)l + 2] = w[2];
                j.lm_state_w[l] = (unsigned char)(st | OV2_LM_3D | OV2_LM_KP3D);
            }
        } else if ((st & OV2_LM_ALIVE) && (st & OV2_LM_KP3D) && a > j.newkf) {
            double rel[7], Tnew[7], Tcw[7], cam[3], w[3];
            const double *Told = M.kf_pose + 7 * (size_t)a;
            se3_mul(j.lb_tmp, Told, rel);
            se3_mul(j.lb_tmp + 7, rel, Tnew);
            se3_inverse(Told, Tcw);
            se3_apply(Tcw, M.lm_xyz + 3 * (size_t)l, cam);          // Frame::projWorldToCam
            se3_apply(Tnew, cam, w);
            j.lm_xyz_w[3 * (size_t)l] = w[0]; j.lm_xyz_w[3 * (size_t)l + 1] = w[1]; j.lm_xyz_w[3 * (size_t)l + 2] = w[2];
            j.lm_state_w[l] = (unsigned char)(st | OV2_LM_3D);
            moved = true;
        }
    }
    lb_count(j, LB_WRITTEN, written);
    lb_count(j, LB_PROP, moved);
}

// launch 4, one lane per keyframe: the solved pose of a non-constant keyframe of the problem (:1533-1548), or
// opt * (ini * old(k)) for a keyframe younger than the loop keyframe (:1560).  A lane reads its own old pose only.
__global__ __launch_bounds__(256) void ml_poses_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    if (!j.lb_on || (int)blockIdx.x * 256 >= M.max_kf) return;   // uniform per workgroup
    const int k = blockIdx.x * 256 + threadIdx.x;
    bool free_ = false, younger = false;
    if (k < M.max_kf) {
        free_ = j.kf_role[k] == 1;   // counted as a free pose of the PROBLEM, alive now or not (only a live one is written)
        if (M.kf_state[k]) {
            if (free_) {
                const flat_out O = flat_of(j, inv);
                const double *T = O.pose + 7 * (size_t)j.kf_idx[k];
#pragma unroll
                for (int q = 0; q < 7; ++q) j.kf_pose_w[7 * (size_t)k + q] = T[q];
            } else if (k > j.newkf) {
                double rel[7], T[7];
                se3_mul(j.lb_tmp, M.kf_pose + 7 * (size_t)k, rel);
                se3_mul(j.lb_tmp + 7, rel, T);
#pragma unroll
                for (int q = 0; q < 7; ++q) j.kf_pose_w[7 * (size_t)k + q] = T[q];
                younger = true;
            }
        }
    }
    lb_count(j, LB_FREE, free_);
    lb_count(j, LB_YOUNGER, younger);
}

// launch 7 (after mu_obs_kernel and mu_recount_kernel: the flagged blocks are gone, observers and oldest observers of the
// problem's landmarks are counted again), one lane per landmark of the problem or of its bad list: the culling over
// set_badlmids (:1623-1650) -- the set-up's isBad() landmarks, launch 3's additions and every landmark with a flagged block
__global__ __launch_bounds__(256) void ml_cull_kernel(const map_job *__restrict__ J, int inv)
{
    const map_job &j = J[blockIdx.y];
    const map_view &M = j.M;
    const int *H = j.hdr;
    if (!j.lb_on) return;
    const int idx = blockIdx.x * 256 + threadIdx.x, NL = H[MH_NLM], NB = H[MH_NBAD];
    bool member = false;
    if (idx < NL + NB) {
        const flat_out O = flat_of(j, inv);
        const int l = idx < NL ? O.lm_lmid[idx] : O.bad_lmid[idx - NL];
        const int st = M.lm_state[l];
        member = idx >= NL || (j.lm_sel[l] & (4 | 8));
        if (member && (st & OV2_LM_ALIVE)) {
            const int nobs = j.lm_nobs[l];
            const bool isobs = st & OV2_LM_OBS;
            const unsigned long long oldest = j.lm_pack[l];
            const int lm_kfid = oldest ? ANCH_TOP - (int)(oldest >> 32) : -1;
            const bool bad = (nobs < 2 && !isobs && (st & OV2_LM_3D)) || (nobs == 0 && !isobs);
            if (bad || (nobs < 3 && lm_kfid < j.newkf - 3 && !isobs)) {
                j.lm_state_w[l] = 0;
                O.rm_lm[atomicAdd(&j.hdr[MH_NRM_LM], 1)] = l;
            }
        }
    }
    lb_count(j, LB_BAD, member);
}

// gathers the headers of all maps (update counts) for one D2H
__global__ __launch_bounds__(64) void mb_hdr_gather_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    if (threadIdx.x < MH_N) j.hdr_out[threadIdx.x] = j.hdr[threadIdx.x];
}

// ov2_map_restore_state_batch: the tables of every map back to their saved state, one launch
__global__ __launch_bounds__(256) void mb_restore_kernel(const map_job *__restrict__ J)
{
    const map_job &j = J[blockIdx.y];
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < 7 * (size_t)j.snap_kf; i += nth) j.kf_pose_w[i] = j.snap_kf_pose[i];
    for (size_t i = tid; i < 3 * (size_t)j.snap_lm; i += nth) j.lm_xyz_w[i] = j.snap_lm_xyz[i];
    for (size_t i = tid; i < (size_t)j.snap_kf; i += nth) j.kf_state_w[i] = j.snap_kf_state[i];
    for (size_t i = tid; i < (size_t)j.snap_lm; i += nth) j.lm_state_w[i] = j.snap_lm_state[i];
    for (size_t i = tid; i < (size_t)j.snap_obs; i += nth) j.obs_flag_w[i] = j.snap_obs_flag[i];
}

map_view view_of(const ov2_map *m)
{
    map_view v;
    v.max_kf = m->max_kf; v.max_lm = m->max_lm; v.n_obs = m->n_obs;
    v.kf_pose = m->kf_pose; v.kf_state = m->kf_state; v.lm_xyz = m->lm_xyz; v.lm_state = m->lm_state;
    v.obs_kf = m->obs_kf; v.obs_lm = m->obs_lm; v.obs_scale = m->obs_scale; v.obs_uv = m->obs_uv; v.obs_ruv = m->obs_ruv;
    v.obs_flag = m->obs_flag;
    v.obs_px = reinterpret_cast<const float2 *>(m->obs_px); v.obs_desc = reinterpret_cast<const uint4 *>(m->obs_desc);
    v.obs_hasdesc = m->obs_hasdesc;
    return v;
}

// one record of the job table
map_job job_of(const ov2_map *m, int newkf, int cur_kfid)
{
    map_job j;
    memset(&j, 0, sizeof(j));
    j.M = view_of(m);
    j.newkf = newkf; j.cur_kfid = cur_kfid;
    j.hdr = m->hdr; j.cov = m->cov; j.kf_role = m->kf_role; j.kf_idx = m->kf_idx; j.lm_nobs = m->lm_nobs; j.lm_sel = m->lm_sel;
    j.lm_anchor = m->lm_anchor; j.lm_flag = m->lm_flag; j.lm_pack = m->lm_pack; j.lm_pidx = m->lm_pidx; j.lm_new = m->lm_new;
    j.obs_cnt = m->obs_cnt; j.obs_off = m->obs_off; j.blk = m->blk;
    j.zero_blk = m->zero_blk; j.zero_vec16 = (unsigned)(m->zero_bytes / 16);
    j.out = m->out_dev; j.out_cap = m->out_cap;
    j.kf_pose_w = m->kf_pose; j.lm_xyz_w = m->lm_xyz; j.kf_state_w = m->kf_state; j.lm_state_w = m->lm_state; j.obs_flag_w = m->obs_flag;
    for (int k = 0; k < 4; ++k) j.K[k] = m->last_K[k];
    j.snap_kf_pose = m->snap_kf_pose; j.snap_lm_xyz = m->snap_lm_xyz; j.snap_kf_state = m->snap_kf_state;
    j.snap_lm_state = m->snap_lm_state; j.snap_obs_flag = m->snap_obs_flag;
    j.snap_kf = m->snap_kf; j.snap_lm = m->snap_lm; j.snap_obs = m->snap_obs;
    j.obs_lm_w = m->obs_lm; j.obs_ruv_w = m->obs_ruv;
    j.obs_desc_w = reinterpret_cast<uint4 *>(m->obs_desc); j.obs_hasdesc_w = m->obs_hasdesc; j.mg_srow = m->mg_srow;
    return j;
}

// The job table of a call lives in the ctx staging block: [B records | B gathered headers].  The records go up with one
// copy; the headers come back with one copy (fetch_headers) into the pinned twin.
struct job_table {
    ov2_ctx *c = nullptr; int B = 0;
    map_job *host = nullptr; const map_job *dev = nullptr;
    int *hdr_host = nullptr, *hdr_dev = nullptr;
    size_t stride = MH_N;                        // ints per map in the gathered copy: the header, then what the stage appends
    unsigned char *tail_host = nullptr, *tail_dev = nullptr;   // tail_bytes of call arguments behind the headers (256-aligned)
    size_t tail_off = 0, tail_bytes = 0;
    ov2_status begin(ov2_ctx *ctx, int nb, int extra_ints = 0, size_t tail = 0)
    {
        c = ctx; B = nb; stride = MH_N + (size_t)extra_ints; tail_bytes = tail;
        void *h, *d;
        const size_t tab = ((size_t)B * sizeof(map_job) + 255) & ~(size_t)255;
        tail_off = (tab + (size_t)B * stride * sizeof(int) + 255) & ~(size_t)255;
        const ov2_status s = ov2_staging(c, tail_off + tail + 256, &h, &d);
        if (s != OV2_OK) return s;
        host = (map_job *)h; dev = (const map_job *)d;
        hdr_host = (int *)((unsigned char *)h + tab); hdr_dev = (int *)((unsigned char *)d + tab);
        tail_host = (unsigned char *)h + tail_off; tail_dev = (unsigned char *)d + tail_off;
        return OV2_OK;
    }
    void set(int b, const map_job &j) { host[b] = j; host[b].hdr_out = hdr_dev + (size_t)b * stride; }
    ov2_status upload()
    {
        // one copy: the records alone, or everything up to the end of the tail when the call has one
        const size_t bytes = tail_bytes ? tail_off + tail_bytes : (size_t)B * sizeof(map_job);
        OV2_HIP(c, hipMemcpyAsync((void *)dev, host, bytes, hipMemcpyHostToDevice, c->stream));
        // calls that return without synchronising leave this copy in flight: the next user of the staging block waits for it
        OV2_HIP(c, hipEventRecord(c->stage_ev, c->stream));
        c->stage_ev_pending = true;
        return OV2_OK;
    }
    ov2_status fetch_headers()   // D2H of the gathered headers + the call's one synchronisation
    {
        OV2_HIP(c, hipMemcpyAsync(hdr_host, hdr_dev, (size_t)B * stride * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        OV2_HIP(c, hipStreamSynchronize(c->stream));
        return OV2_OK;
    }
};

template <typename T>
ov2_status exclusive_scan(ov2_ctx *c, const job_table &T_, int which, int n_max)
{
    if (n_max <= 0) return OV2_OK;   // the totals already hold the zeros of the cleared header
    const dim3 g((n_max + 1023) / 1024, T_.B);
    OV2_LAUNCH(c, OV2_K_MAP, scan_block_kernel<T>, g, dim3(1024), 0, c->stream, T_.dev, which);
    OV2_LAUNCH(c, OV2_K_MAP, scan_top_kernel<T>, dim3(1, T_.B), dim3(1024), 0, c->stream, T_.dev, which);
    OV2_LAUNCH(c, OV2_K_MAP, scan_add_kernel<T>, g, dim3(1024), 0, c->stream, T_.dev, which);
    return OV2_OK;
}

template <typename T>
ov2_status dmalloc(ov2_ctx *c, T **p, size_t count)
{
    hipError_t e = hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "map table hipMalloc(%zu): %s", count * sizeof(T), hipGetErrorString(e));
    return OV2_OK;
}

// stage `count` elements of each host array behind each other in the ctx staging block; returns device pointers
struct stager {
    ov2_ctx *c; unsigned char *h = nullptr, *d = nullptr; size_t off = 0, cap = 0;
    ov2_status begin(size_t bytes)
    {
        void *hh, *dd;
        ov2_status s = ov2_staging(c, bytes + 256, &hh, &dd);
        if (s != OV2_OK) return s;
        h = (unsigned char *)hh; d = (unsigned char *)dd; cap = bytes + 256; off = 0;
        return OV2_OK;
    }
    template <typename T> const T *put(const T *src, size_t count)
    {
        if (!src) return nullptr;
        off = (off + 15) & ~(size_t)15;
        memcpy(h + off, src, count * sizeof(T));
        const T *dp = reinterpret_cast<const T *>(d + off);
        off += count * sizeof(T);
        return dp;
    }
    ov2_status flush() { OV2_HIP(c, hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, c->stream)); return OV2_OK; }
};

}  // namespace

// every device array whose size follows the capacities (tables + set-up scratch); pointers must be null on entry
static ov2_status alloc_tables(ov2_map *m)
{
    ov2_ctx *c = m->c;
    ov2_status s = OV2_OK;
    const size_t K = m->max_kf, L = m->max_lm, N = m->max_obs;
#define A(p, n) if (s == OV2_OK) s = dmalloc(c, &m->p, (n))
    A(kf_pose, 7 * K); A(kf_state, K); A(lm_xyz, 3 * L); A(lm_state, L);
    A(obs_kf, N); A(obs_lm, N); A(obs_scale, N); A(obs_uv, 2 * N); A(obs_ruv, 2 * N); A(obs_flag, N);
    A(kf_idx, K); A(lm_flag, L); A(lm_pack, L); A(lm_pidx, L);
    m->zero_bytes = (sizeof(int) * (MH_N + 2 * K + 3 * L) + L + 15) & ~(size_t)15;   // cleared 16 bytes at a time
    A(zero_blk, m->zero_bytes);
    if (s == OV2_OK) {
        int *z = reinterpret_cast<int *>(m->zero_blk);
        m->hdr = z; m->cov = z + MH_N; m->kf_role = m->cov + K; m->lm_nobs = m->kf_role + K; m->lm_sel = m->lm_nobs + L;
        m->lm_anchor = m->lm_sel + L;
        m->lm_new = reinterpret_cast<unsigned char *>(m->lm_anchor + L);
    }
    A(obs_cnt, N); A(obs_off, N); A(blk, 2 * ((std::max(std::max(N, L), K) + 1023) / 1024 + 1));   // block sums, up to 64-bit
    m->tt_zero_bytes = (sizeof(int) * (MH_N + 3 * L) + 15) & ~(size_t)15;
    A(tt_zero, m->tt_zero_bytes); A(tt_int, 3 * L); A(tt_dbl, 4 * L);
    if (s == OV2_OK) {
        m->tt_nobs = reinterpret_cast<int *>(m->tt_zero) + MH_N; m->tt_old = m->tt_nobs + L; m->tt_nrow = m->tt_old + L;
    }
    m->ts_zero_bytes = (sizeof(int) * (MH_N + L) + 15) & ~(size_t)15;
    A(ts_zero, m->ts_zero_bytes); A(ts_int, 2 * L); A(ts_dbl, 4 * L); A(ts_why, L);
    if (s == OV2_OK) m->ts_mark = reinterpret_cast<int *>(m->ts_zero) + MH_N;
    m->fl_zero_bytes = (sizeof(int) * (MH_N + L + 4 * K) + L + 15) & ~(size_t)15;
    A(fl_zero, m->fl_zero_bytes); A(fl_start, K); A(fl_rows, N); A(fl_unset, L);
    if (s == OV2_OK) {
        m->fl_nobs = reinterpret_cast<int *>(m->fl_zero) + MH_N; m->fl_cov = m->fl_nobs + L; m->fl_n3d = m->fl_cov + K;
        m->fl_cnt = m->fl_n3d + K; m->fl_fill = m->fl_cnt + K;
        m->fl_new = reinterpret_cast<unsigned char *>(m->fl_fill + K);
    }
    m->mg_zero_bytes = (sizeof(int) * (MH_N + 3 * L + K) + L + 15) & ~(size_t)15;
    A(mg_zero, m->mg_zero_bytes); A(mg_start, L); A(mg_rows, N);
    if (s == OV2_OK) {
        m->mg_cnt = reinterpret_cast<int *>(m->mg_zero) + MH_N; m->mg_fill = m->mg_cnt + L; m->mg_next = m->mg_fill + L;
        m->mg_stamp = m->mg_next + L;
        m->mg_mark = reinterpret_cast<unsigned char *>(m->mg_stamp + K);
    }
#undef A
    return s;
}

// the match columns at the current capacities (ov2_map_enable_match_columns, and every growth of a map that has them): no row
// carries a descriptor, every pixel is 0; pointers must be null on entry
static ov2_status alloc_match_columns(ov2_map *m)
{
    ov2_ctx *c = m->c;
    ov2_status s = OV2_OK;
    const size_t K = m->max_kf, L = m->max_lm, N = m->max_obs;
    if (s == OV2_OK) s = dmalloc(c, &m->obs_px, 2 * N);
    if (s == OV2_OK) s = dmalloc(c, &m->obs_desc, 32 * N);   // hipMalloc aligns far beyond the 16 bytes the lane copies need
    if (s == OV2_OK) s = dmalloc(c, &m->obs_hasdesc, N);
    if (s == OV2_OK) s = dmalloc(c, &m->mg_srow, K);
    if (s == OV2_OK && !(m->gt_seen_h = (int *)calloc(std::max<size_t>(L, 1), sizeof(int))))
        s = ov2_set_err(c, OV2_ERR_NOMEM, "map landmark list of %zu entries", L);
    m->gt_gen = 0;
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemsetAsync(m->obs_px, 0, 2 * std::max<size_t>(N, 1) * sizeof(float), c->stream));
    OV2_HIP(c, hipMemsetAsync(m->obs_hasdesc, 0, std::max<size_t>(N, 1), c->stream));
    return OV2_OK;
}

static void free_match_columns(ov2_map *m)
{
    void *dev[] = {m->obs_px, m->obs_desc, m->obs_hasdesc, m->mg_srow};
    for (void *p : dev) if (p) (void)hipFree(p);
    free(m->gt_seen_h);
    m->obs_px = nullptr; m->obs_desc = m->obs_hasdesc = nullptr; m->mg_srow = nullptr; m->gt_seen_h = nullptr;
}

// the per-keyframe tables of the local id sets and the scratch of ov2_map_local_ids_batch at the current capacities
// (ov2_map_enable_local_sets, and every growth of a map that has them): no keyframe has a set; pointers must be null on entry.
// The id pool does not follow the capacities and is not touched here.
static ov2_status alloc_local_sets(ov2_map *m)
{
    ov2_ctx *c = m->c;
    ov2_status s = OV2_OK;
    const size_t K = m->max_kf, L = m->max_lm;
    if (s == OV2_OK) s = dmalloc(c, &m->ls_start, K);
    if (s == OV2_OK) s = dmalloc(c, &m->ls_count, K);
    if (s == OV2_OK) s = dmalloc(c, &m->ls_pos, L);
    m->ls_zero_bytes = (sizeof(int) * (MH_N + K + L) + L + 15) & ~(size_t)15;
    if (s == OV2_OK) s = dmalloc(c, &m->ls_zero, m->ls_zero_bytes);
    if (s == OV2_OK) {
        m->ls_cov = reinterpret_cast<int *>(m->ls_zero) + MH_N; m->ls_mark = m->ls_cov + K;
        m->ls_obs = reinterpret_cast<unsigned char *>(m->ls_mark + L);
        m->ls_start_h = (int *)calloc(std::max<size_t>(K, 1), sizeof(int));
        m->ls_count_h = (int *)calloc(std::max<size_t>(K, 1), sizeof(int));
        if (!m->ls_start_h || !m->ls_count_h) s = ov2_set_err(c, OV2_ERR_NOMEM, "map local-set tables of %zu entries", K);
    }
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemsetAsync(m->ls_start, 0, K * sizeof(int), c->stream));
    OV2_HIP(c, hipMemsetAsync(m->ls_count, 0, K * sizeof(int), c->stream));
    return OV2_OK;
}

static void free_local_sets(ov2_map *m)
{
    void *dev[] = {m->ls_start, m->ls_count, m->ls_pos, m->ls_zero};
    for (void *p : dev) if (p) (void)hipFree(p);
    free(m->ls_start_h); free(m->ls_count_h);
    m->ls_start = m->ls_count = m->ls_pos = m->ls_cov = m->ls_mark = nullptr; m->ls_zero = m->ls_obs = nullptr;
    m->ls_start_h = m->ls_count_h = nullptr;
}

static void free_capacity_arrays(ov2_map *m)
{
    free_match_columns(m);
    free_local_sets(m);
    void *dev[] = {m->kf_pose, m->kf_state, m->lm_xyz, m->lm_state, m->obs_kf, m->obs_lm, m->obs_scale, m->obs_uv, m->obs_ruv,
                   m->obs_flag, m->zero_blk, m->kf_idx, m->lm_flag, m->lm_pack, m->lm_pidx, m->obs_cnt, m->obs_off, m->blk,
                   m->tt_zero, m->tt_int, m->tt_dbl, m->ts_zero, m->ts_int, m->ts_dbl, m->ts_why,
                   m->fl_zero, m->fl_start, m->fl_rows, m->fl_unset,
                   m->mg_zero, m->mg_start, m->mg_rows};
    for (void *p : dev) if (p) (void)hipFree(p);
}

// The tables grow by doubling when an id or the observation count passes the capacity: fresh arrays, device copies of
// the live prefixes, old arrays freed (a rare event; one synchronisation).
static ov2_status ensure_capacity(ov2_map *m, int need_kf, int need_lm, int need_obs)
{
    if (need_kf <= m->max_kf && need_lm <= m->max_lm && need_obs <= m->max_obs) return OV2_OK;
    ov2_ctx *c = m->c;
    ov2_map old = *m;
    auto grown = [](int have, int need) { return need <= have ? have : std::max(need, have + have / 2 + 16); };
    m->max_kf = grown(old.max_kf, need_kf); m->max_lm = grown(old.max_lm, need_lm); m->max_obs = grown(old.max_obs, need_obs);
    m->kf_pose = nullptr; m->kf_state = nullptr; m->lm_xyz = nullptr; m->lm_state = nullptr;
    m->obs_kf = m->obs_lm = m->obs_scale = nullptr; m->obs_uv = m->obs_ruv = nullptr; m->obs_flag = nullptr;
    m->zero_blk = nullptr; m->kf_idx = m->lm_flag = m->obs_cnt = m->obs_off = m->blk = nullptr; m->lm_pack = m->lm_pidx = nullptr;
    m->tt_zero = nullptr; m->tt_int = nullptr; m->tt_dbl = nullptr;
    m->ts_zero = nullptr; m->ts_int = nullptr; m->ts_dbl = nullptr; m->ts_why = nullptr;
    m->fl_zero = nullptr; m->fl_start = m->fl_rows = m->fl_unset = nullptr;
    m->mg_zero = nullptr; m->mg_start = m->mg_rows = nullptr;
    m->obs_px = nullptr; m->obs_desc = m->obs_hasdesc = nullptr; m->mg_srow = nullptr; m->gt_seen_h = nullptr;
    m->ls_start = m->ls_count = m->ls_pos = m->ls_cov = m->ls_mark = nullptr; m->ls_zero = m->ls_obs = nullptr;
    m->ls_start_h = m->ls_count_h = nullptr;
    ov2_status s = alloc_tables(m);
    if (s == OV2_OK && old.obs_hasdesc) s = alloc_match_columns(m);   // a map that has the columns keeps them
    if (s == OV2_OK && old.ls_on) s = alloc_local_sets(m);            // ... and one that has the local sets keeps those (the pool stays)
    unsigned char *alive = s == OV2_OK ? (unsigned char *)calloc((size_t)m->max_kf, 1) : nullptr;
    if (s == OV2_OK && !alive) s = ov2_set_err(c, OV2_ERR_NOMEM, "map keyframe list of %d entries", m->max_kf);
    if (s != OV2_OK) {
        free_capacity_arrays(m);
        *m = old;
        return s;
    }
    memcpy(alive, old.kf_alive_h, (size_t)old.max_kf);
    free(old.kf_alive_h);
    m->kf_alive_h = alive;
    hipStream_t st = c->stream;
    const size_t K = old.max_kf, L = old.max_lm, N = old.n_obs;
    OV2_HIP(c, hipMemsetAsync(m->kf_state, 0, (size_t)m->max_kf, st));
    OV2_HIP(c, hipMemsetAsync(m->lm_state, 0, (size_t)m->max_lm, st));
    OV2_HIP(c, hipMemsetAsync(m->obs_flag, 0, (size_t)m->max_obs, st));
#define CP(p, n) if ((n) > 0) OV2_HIP(c, hipMemcpyAsync(m->p, old.p, (n) * sizeof(*m->p), hipMemcpyDeviceToDevice, st))
    CP(kf_pose, 7 * K); CP(kf_state, K); CP(lm_xyz, 3 * L); CP(lm_state, L);
    CP(obs_kf, N); CP(obs_lm, N); CP(obs_scale, N); CP(obs_uv, 2 * N); CP(obs_ruv, 2 * N); CP(obs_flag, N);
    if (old.obs_hasdesc) { CP(obs_px, 2 * N); CP(obs_desc, 32 * N); CP(obs_hasdesc, N); }
    if (old.ls_on) {   // the per-keyframe columns of the local sets travel with the keyframe capacity
        CP(ls_start, K); CP(ls_count, K);
        memcpy(m->ls_start_h, old.ls_start_h, K * sizeof(int)); memcpy(m->ls_count_h, old.ls_count_h, K * sizeof(int));
    }
#undef CP
    OV2_HIP(c, hipStreamSynchronize(st));
    free_capacity_arrays(&old);
    // the scratch arrays of the last set-up and a saved state belong to the old capacities
    m->last_valid = 0;
    void *snap[] = {m->snap_kf_pose, m->snap_lm_xyz, m->snap_kf_state, m->snap_lm_state, m->snap_obs_flag};
    for (void *p : snap) if (p) (void)hipFree(p);
    m->snap_kf_pose = m->snap_lm_xyz = nullptr; m->snap_kf_state = m->snap_lm_state = m->snap_obs_flag = nullptr;
    m->snap_kf = m->snap_lm = m->snap_obs = 0; m->snap_floor = 0;
    free(m->snap_kf_alive_h); m->snap_kf_alive_h = nullptr;
    return OV2_OK;
}

// fewer than half of >= MAP_COMPACT_MIN_ROWS rows live (and, with a saved state, more than twice the rows its last squeeze kept)
static bool squeeze_due(const ov2_map *m, long long live)
{
    return m->n_obs >= MAP_COMPACT_MIN_ROWS && 2 * std::max(live, (long long)m->snap_floor) < m->n_obs;
}

// squeezes the dead rows out of the observation table (stable); one synchronisation, fresh column arrays of the same capacity
static ov2_status compact_obs(ov2_map *m)
{
    ov2_ctx *c = m->c;
    hipStream_t st = c->stream;
    const int N = m->n_obs;
    if (N <= 0) return OV2_OK;
    // the fresh column arrays are released on every early return, kept once they have replaced the old ones
    struct fresh_cols {
        obs_cols O = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool committed = false;
        ~fresh_cols()
        {
            if (committed) return;
            void *p[] = {O.kf, O.lm, O.scale, O.uv, O.ruv, O.flag, O.snap_flag, O.px, O.desc, O.hasdesc};
            for (void *q : p) if (q) (void)hipFree(q);
        }
    } F;
    obs_cols &O = F.O;
    const size_t cap = (size_t)m->max_obs;
    ov2_status s = OV2_OK;
#define A(p, n) if (s == OV2_OK) s = dmalloc(c, &O.p, (n))
    A(kf, cap); A(lm, cap); A(scale, cap); A(uv, 2 * cap); A(ruv, 2 * cap); A(flag, cap);
    // a saved state of exactly these rows and capacities (the only one ov2_map_restore_state_batch accepts) survives
    const bool keep_snap = m->snap_kf_pose && m->snap_obs_flag && m->snap_obs == N && m->snap_kf == m->max_kf && m->snap_lm == m->max_lm;
    if (keep_snap) A(snap_flag, (size_t)N);
    if (m->obs_hasdesc) { A(px, 2 * cap); A(desc, 32 * cap); A(hasdesc, cap); }
#undef A
    if (s != OV2_OK) return s;
    const map_view M = view_of(m);
    const snap_view SV = {m->snap_kf_state, m->snap_lm_state, keep_snap ? m->snap_obs_flag : nullptr};
    const dim3 g((N + 255) / 256), b(256);
    job_table JT;
    if ((s = JT.begin(c, 1)) != OV2_OK) return s;
    JT.set(0, job_of(m, -1, -1));
    if ((s = JT.upload()) != OV2_OK) return s;
    OV2_HIP(c, hipMemsetAsync(O.flag, 0, cap, st));
    if (O.hasdesc) {   // rows beyond the squeezed ones: as ov2_map_enable_match_columns leaves them
        OV2_HIP(c, hipMemsetAsync(O.hasdesc, 0, cap, st));
        OV2_HIP(c, hipMemsetAsync(O.px, 0, 2 * cap * sizeof(float), st));
    }
    OV2_LAUNCH(c, OV2_K_MAP, mc_mark_kernel, g, b, 0, st, M, SV, m->obs_cnt);
    if ((s = exclusive_scan<int>(c, JT, SC_LIVE, N)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mc_scatter_kernel, g, b, 0, st, M, SV.obs_flag, (const int *)m->obs_cnt, (const int *)m->obs_off, O);
    OV2_HIP(c, hipMemcpyAsync(m->hdr_host, m->hdr, MH_N * sizeof(int), hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    void *old[] = {m->obs_kf, m->obs_lm, m->obs_scale, m->obs_uv, m->obs_ruv, m->obs_flag};
    for (void *p : old) (void)hipFree(p);
    m->obs_kf = O.kf; m->obs_lm = O.lm; m->obs_scale = O.scale; m->obs_uv = O.uv; m->obs_ruv = O.ruv; m->obs_flag = O.flag;
    if (O.hasdesc) {
        void *oldc[] = {m->obs_px, m->obs_desc, m->obs_hasdesc};
        for (void *p : oldc) (void)hipFree(p);
        m->obs_px = O.px; m->obs_desc = O.desc; m->obs_hasdesc = O.hasdesc;
    }
    F.committed = true;
    m->n_obs = m->hdr_host[MH_NLIVE];
    m->n_compactions++;
    m->last_valid = 0;   // the row indices of the last set-up's scratch arrays are gone
    m->live_rows = m->n_obs; m->live_known = 1;
    if (m->snap_obs_flag) (void)hipFree(m->snap_obs_flag);
    if (keep_snap) {   // the saved flags, squeezed like the rows
        m->snap_obs_flag = O.snap_flag; m->snap_obs = m->n_obs;
        m->snap_floor = m->n_obs;   // rows that only the saved state keeps alive must not trigger a squeeze at every set-up
    } else if (m->snap_obs_flag) {  // a saved state of other rows: it could not be restored before, it cannot now
        m->snap_obs_flag = nullptr; m->snap_obs = -1; m->snap_floor = 0;
    }
    return OV2_OK;
}

extern "C" ov2_status ov2_map_compact(ov2_map *m, int *rows_before, int *rows_after)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    OV2_HIP(m->c, hipSetDevice(m->c->device));
    if (rows_before) *rows_before = m->n_obs;
    const ov2_status s = compact_obs(m);
    if (rows_after) *rows_after = m->n_obs;
    return s;
}

extern "C" ov2_status ov2_map_obs_rows(const ov2_map *m, int *rows, int *capacity, int *compactions)
{
    if (!m) return OV2_ERR_INVALID;
    if (rows) *rows = m->n_obs;
    if (capacity) *capacity = m->max_obs;
    if (compactions) *compactions = m->n_compactions;
    return OV2_OK;
}

extern "C" ov2_status ov2_map_create(ov2_ctx *c, int max_kf, int max_lm, int max_obs, ov2_map **out)
{
    if (!c || !out || max_kf <= 0 || max_lm <= 0 || max_obs <= 0) return OV2_ERR_INVALID;
    *out = nullptr;
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_map *m = new (std::nothrow) ov2_map();
    if (!m) return OV2_ERR_NOMEM;
    memset(m, 0, sizeof(*m));
    m->c = c; m->max_kf = max_kf; m->max_lm = max_lm; m->max_obs = max_obs;
    ov2_status s = alloc_tables(m);
    if (s == OV2_OK && !(m->kf_alive_h = (unsigned char *)calloc((size_t)max_kf, 1))) s = ov2_set_err(c, OV2_ERR_NOMEM, "map keyframe list");
    if (s == OV2_OK && hipHostMalloc((void **)&m->hdr_host, MH_N * sizeof(int), hipHostMallocDefault) != hipSuccess)
        s = ov2_set_err(c, OV2_ERR_NOMEM, "map header hipHostMalloc");
    if (s != OV2_OK) { ov2_map_destroy(m); return s; }
    OV2_HIP(c, hipMemsetAsync(m->kf_state, 0, (size_t)max_kf, c->stream));
    OV2_HIP(c, hipMemsetAsync(m->lm_state, 0, (size_t)max_lm, c->stream));
    OV2_HIP(c, hipMemsetAsync(m->obs_flag, 0, (size_t)max_obs, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    { std::lock_guard<std::mutex> g(c->mu); c->maps.push_back(m); }
    *out = m;
    return OV2_OK;
}

static void free_tables(ov2_map *m)
{
    free_capacity_arrays(m);
    void *snap[] = {m->snap_kf_pose, m->snap_lm_xyz, m->snap_kf_state, m->snap_lm_state, m->snap_obs_flag};
    for (void *p : snap) if (p) (void)hipFree(p);
    if (m->out_dev) (void)hipFree(m->out_dev);
    if (m->out_host) (void)hipHostFree(m->out_host);
    if (m->hdr_host) (void)hipHostFree(m->hdr_host);
    if (m->fl_removed_h) (void)hipHostFree(m->fl_removed_h);
    if (m->sb_ws) (void)hipFree(m->sb_ws);
    if (m->ls_pool) (void)hipFree(m->ls_pool);
    if (m->ls_out_h) (void)hipHostFree(m->ls_out_h);
    free(m->kf_alive_h); free(m->snap_kf_alive_h);
}

void ov2_map_orphan(ov2_map *m)
{
    free_tables(m);
    ov2_ctx *none = nullptr;
    ov2_map blank;
    memset(&blank, 0, sizeof(blank));
    *m = blank;
    m->c = none;
}

extern "C" void ov2_map_destroy(ov2_map *m)
{
    if (!m) return;
    if (m->c) {   // c == nullptr: the ctx went first and already released the tables
        ov2_ctx *c = m->c;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        free_tables(m);
        std::lock_guard<std::mutex> g(c->mu);
        c->maps.erase(std::remove(c->maps.begin(), c->maps.end(), m), c->maps.end());
    }
    delete m;
}

extern "C" ov2_status ov2_map_enable_match_columns(ov2_map *m)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    if (m->obs_hasdesc) return OV2_OK;
    ov2_ctx *c = m->c;
    OV2_HIP(c, hipSetDevice(c->device));
    const ov2_status s = alloc_match_columns(m);
    if (s != OV2_OK) { free_match_columns(m); return s; }
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

// ---- the per-keyframe local id sets (Frame::set_local_mapids_) -------------------------------------------------------------
// Sets are appended to the pool; a replaced set and the set of a removed keyframe stay behind as garbage.  The pool is
// squeezed under the observation table's rule (squeeze_due): fewer than half of >= MAP_COMPACT_MIN_ROWS appended entries
// belong to a set that counts.
static bool ls_squeeze_due(const ov2_map *m)
{
    return m->ls_pool_used >= MAP_COMPACT_MIN_ROWS && 2ll * m->ls_live < (long long)m->ls_pool_used;
}

// room for `need` more entries behind the used part of the pool, before anything that appends is enqueued: a squeeze when one
// is due (the sets that count, in ascending kfid, into a fresh pool), a larger pool when it is still short (a rare event;
// one synchronisation either way)
static ov2_status ls_reserve(ov2_map *m, int need)
{
    ov2_ctx *c = m->c;
    const bool squeeze = ls_squeeze_due(m);
    const long long used = squeeze ? m->ls_live : m->ls_pool_used;
    if (!squeeze && used + need <= m->ls_pool_cap) return OV2_OK;
    long long cap = m->ls_pool_cap;
    if (used + need > cap) cap = std::max(used + need, cap + cap / 2 + 16);
    if (cap > 0x7fffffffll) return ov2_set_err(c, OV2_ERR_NOMEM, "local-set pool of %lld entries", cap);
    int *fresh = nullptr;
    ov2_status s = dmalloc(c, &fresh, (size_t)cap);
    if (s != OV2_OK) return s;
    hipStream_t st = c->stream;
    std::vector<int> start;
    hipError_t e = hipSuccess;
    if (squeeze) {
        start.assign((size_t)m->max_kf, 0);
        int o = 0;
        for (int k = 0; k < m->max_kf && e == hipSuccess; ++k) {
            const int n = m->ls_count_h[k];
            if (!n) continue;
            e = hipMemcpyAsync(fresh + o, m->ls_pool + m->ls_start_h[k], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st);
            start[k] = o; o += n;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(m->ls_start, start.data(), (size_t)m->max_kf * sizeof(int), hipMemcpyHostToDevice, st);
    } else if (m->ls_pool_used) {
        e = hipMemcpyAsync(fresh, m->ls_pool, (size_t)m->ls_pool_used * sizeof(int), hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        return ov2_set_err(c, OV2_ERR_HIP, "local-set pool copy failed: %s", hipGetErrorString(e));
    }
    if (m->ls_pool) (void)hipFree(m->ls_pool);
    m->ls_pool = fresh; m->ls_pool_cap = (int)cap;
    if (squeeze) {
        memcpy(m->ls_start_h, start.data(), (size_t)m->max_kf * sizeof(int));
        m->ls_pool_used = m->ls_live;
        m->ls_squeezes++;
    }
    return OV2_OK;
}

// the set of a keyframe that left the map: unreadable from here on, its entries garbage
static ov2_status ls_forget(ov2_map *m, int kfid)
{
    if (!m->ls_on || !m->ls_count_h[kfid]) return OV2_OK;
    m->ls_live -= m->ls_count_h[kfid];
    m->ls_count_h[kfid] = 0;
    OV2_HIP(m->c, hipMemsetAsync(m->ls_count + kfid, 0, sizeof(int), m->c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_map_enable_local_sets(ov2_map *m, int pool_hint)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (pool_hint < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_enable_local_sets: negative pool size %d", pool_hint);
    if (m->ls_on) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_status s = alloc_local_sets(m);
    if (s == OV2_OK) s = dmalloc(c, &m->ls_pool, (size_t)pool_hint);
    if (s != OV2_OK) {
        free_local_sets(m);
        if (m->ls_pool) (void)hipFree(m->ls_pool);
        m->ls_pool = nullptr;
        return s;
    }
    m->ls_pool_cap = pool_hint; m->ls_pool_used = m->ls_live = m->ls_squeezes = 0;
    m->ls_on = 1;
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_map_local_pool(const ov2_map *m, int *used, int *capacity, int *live, int *squeezes)
{
    if (!m || !m->ls_on) return OV2_ERR_INVALID;
    if (used) *used = m->ls_pool_used;
    if (capacity) *capacity = m->ls_pool_cap;
    if (live) *live = m->ls_live;
    if (squeezes) *squeezes = m->ls_squeezes;
    return OV2_OK;
}

extern "C" ov2_status ov2_map_set_local_set(ov2_map *m, int kfid, int n, const int32_t *lmid)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (!m->ls_on) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_local_set: the map has no local sets");
    if (n < 0 || (n && !lmid)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_local_set: null argument");
    if (kfid < 0 || kfid >= m->max_kf || !m->kf_alive_h[kfid]) return ov2_set_err(c, OV2_ERR_INVALID, "keyframe %d is not alive in the map", kfid);
    std::vector<int32_t> ids(lmid, lmid + n);
    std::sort(ids.begin(), ids.end());
    if (n && ids[0] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative lmid %d", ids[0]);
    // the landmark tables grow to cover the largest id (below): one stray id must not ask for gigabytes
    if (n && (long long)ids[n - 1] >= (long long)m->max_lm + OV2_LOCAL_SET_LMID_SPAN)
        return ov2_set_err(c, OV2_ERR_INVALID, "lmid %d lies too far beyond the landmark capacity %d", ids[n - 1], m->max_lm);
    for (int i = 1; i < n; ++i)
        if (ids[i] == ids[i - 1]) return ov2_set_err(c, OV2_ERR_INVALID, "lmid %d appears twice in the set", ids[i]);
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_status s;
    // a stored id indexes the per-landmark marks of ov2_map_local_ids_batch: the landmark capacity covers it
    if (n && (s = ensure_capacity(m, m->max_kf, ids[n - 1] + 1, m->n_obs)) != OV2_OK) return s;
    if ((s = ls_reserve(m, n)) != OV2_OK) return s;
    stager S{c};
    if ((s = S.begin((size_t)n * sizeof(int) + 64)) != OV2_OK) return s;
    const int entry[2] = {m->ls_pool_used, n};
    const int *de = S.put(entry, 2), *dl = S.put(ids.data(), (size_t)n);
    if ((s = S.flush()) != OV2_OK) return s;
    hipStream_t st = c->stream;
    if (n) OV2_HIP(c, hipMemcpyAsync(m->ls_pool + m->ls_pool_used, dl, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemcpyAsync(m->ls_start + kfid, de, sizeof(int), hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemcpyAsync(m->ls_count + kfid, de + 1, sizeof(int), hipMemcpyDeviceToDevice, st));
    m->ls_live += n - m->ls_count_h[kfid];
    m->ls_start_h[kfid] = m->ls_pool_used; m->ls_count_h[kfid] = n;
    m->ls_pool_used += n;
    OV2_HIP(c, hipStreamSynchronize(st));   // the staging block is free again
    return OV2_OK;
}

extern "C" ov2_status ov2_map_get_local_set(ov2_map *m, int kfid, int cap, int32_t *lmid, int *n)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (!m->ls_on) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_get_local_set: the map has no local sets");
    if (!n || cap < 0 || (cap && !lmid)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_get_local_set: null argument");
    if (kfid < 0 || kfid >= m->max_kf || !m->kf_alive_h[kfid]) return ov2_set_err(c, OV2_ERR_INVALID, "keyframe %d is not alive in the map", kfid);
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    *n = m->ls_count_h[kfid];
    const int take = std::min(cap, *n);
    if (take > 0) OV2_HIP(c, hipMemcpy(lmid, m->ls_pool + m->ls_start_h[kfid], (size_t)take * sizeof(int), hipMemcpyDeviceToHost));
    return OV2_OK;
}

// px (n x 2 floats) / desc (n x 32) / has_desc (n) are read on a map with the match columns only; null there = pixel 0 / no descriptor
static ov2_status add_keyframe_impl(ov2_map *m, int kfid, const double *Twc, int n, const int32_t *lmid, const double *unpx,
                                    const double *runpx, const uint8_t *is_stereo, const int32_t *scale, const float *px,
                                    const uint8_t *desc, const uint8_t *has_desc)
{
    ov2_ctx *c = m->c;
    if (!Twc || n < 0 || (n && (!lmid || !unpx))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_add_keyframe: null argument");
    if (kfid < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative kfid %d", kfid);
    int top_lm = -1;
    for (int i = 0; i < n; ++i) {
        if (lmid[i] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative lmid %d", lmid[i]);
        top_lm = std::max(top_lm, lmid[i]);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    {
        const ov2_status gs = ensure_capacity(m, kfid + 1, top_lm + 1, m->n_obs + n);
        if (gs != OV2_OK) return gs;
    }
    // the rows are appended as they are: assemble them in the staging block, then plain copies into the tables
    stager S{c};
    const bool cols = m->obs_hasdesc != nullptr;
    if (!(desc && has_desc)) desc = has_desc = nullptr;
    ov2_status s = S.begin((size_t)n * (3 * sizeof(int) + 4 * sizeof(double) + 1 + (cols ? 2 * sizeof(float) + 33 : 0)) + 7 * sizeof(double) + 512);
    if (s != OV2_OK) return s;
    const double *dT = S.put(Twc, 7);
    const int *dl = S.put(lmid, n);
    const double *du = S.put(unpx, 2 * (size_t)n);
    const float *dpx = cols ? S.put(px, 2 * (size_t)n) : nullptr;
    const uint8_t *ddesc = cols ? S.put(desc, 32 * (size_t)n) : nullptr, *dhas = cols ? S.put(has_desc, (size_t)n) : nullptr;
    // derived columns are built in place in the pinned block
    S.off = (S.off + 15) & ~(size_t)15;
    int *hk = reinterpret_cast<int *>(S.h + S.off); const int *dk = reinterpret_cast<const int *>(S.d + S.off); S.off += sizeof(int) * n;
    S.off = (S.off + 15) & ~(size_t)15;
    int *hs = reinterpret_cast<int *>(S.h + S.off); const int *ds = reinterpret_cast<const int *>(S.d + S.off); S.off += sizeof(int) * n;
    S.off = (S.off + 15) & ~(size_t)15;
    double *hr = reinterpret_cast<double *>(S.h + S.off); const double *dr = reinterpret_cast<const double *>(S.d + S.off); S.off += sizeof(double) * 2 * n;
    S.off = (S.off + 15) & ~(size_t)15;
    unsigned char *hf = S.h + S.off; const unsigned char *df = S.d + S.off; S.off += n;
    for (int i = 0; i < n; ++i) {
        hk[i] = kfid;
        hs[i] = scale ? scale[i] : 0;
        const bool st = is_stereo && is_stereo[i] && runpx;
        hr[2 * i] = st ? runpx[2 * i] : 0.0; hr[2 * i + 1] = st ? runpx[2 * i + 1] : 0.0;
        hf[i] = OBS_ALIVE | (st ? OBS_STEREO : 0);
    }
    if ((s = S.flush()) != OV2_OK) return s;
    const size_t o = m->n_obs;
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(m->kf_pose + 7 * (size_t)kfid, dT, 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemsetAsync(m->kf_state + kfid, 1, 1, st));
    if (n) {
        OV2_HIP(c, hipMemcpyAsync(m->obs_lm + o, dl, sizeof(int) * n, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(m->obs_uv + 2 * o, du, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(m->obs_kf + o, dk, sizeof(int) * n, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(m->obs_scale + o, ds, sizeof(int) * n, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(m->obs_ruv + 2 * o, dr, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(m->obs_flag + o, df, n, hipMemcpyDeviceToDevice, st));
        if (cols) {   // the slots may have held rows that a squeeze moved away
            if (dpx) OV2_HIP(c, hipMemcpyAsync(m->obs_px + 2 * o, dpx, sizeof(float) * 2 * n, hipMemcpyDeviceToDevice, st));
            else OV2_HIP(c, hipMemsetAsync(m->obs_px + 2 * o, 0, sizeof(float) * 2 * n, st));
            if (ddesc) {
                OV2_HIP(c, hipMemcpyAsync(m->obs_desc + 32 * o, ddesc, 32 * (size_t)n, hipMemcpyDeviceToDevice, st));
                OV2_HIP(c, hipMemcpyAsync(m->obs_hasdesc + o, dhas, n, hipMemcpyDeviceToDevice, st));
            } else OV2_HIP(c, hipMemsetAsync(m->obs_hasdesc + o, 0, n, st));
        }
    }
    m->n_obs += n;
    m->kf_alive_h[kfid] = 1;
    OV2_HIP(c, hipStreamSynchronize(st));   // the staging block is free again
    return OV2_OK;
}

extern "C" ov2_status ov2_map_add_keyframe(ov2_map *m, int kfid, const double *Twc, int n, const int32_t *lmid,
                                           const double *unpx, const double *runpx, const uint8_t *is_stereo,
                                           const int32_t *scale)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    return add_keyframe_impl(m, kfid, Twc, n, lmid, unpx, runpx, is_stereo, scale, nullptr, nullptr, nullptr);
}

extern "C" ov2_status ov2_map_add_keyframe_px(ov2_map *m, int kfid, const double *Twc, int n, const int32_t *lmid,
                                              const double *unpx, const double *runpx, const uint8_t *is_stereo,
                                              const int32_t *scale, const float *px, const uint8_t *desc, const uint8_t *has_desc)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    if (!m->obs_hasdesc) return ov2_set_err(m->c, OV2_ERR_INVALID, "ov2_map_add_keyframe_px: the map has no match columns");
    if (n > 0 && !px) return ov2_set_err(m->c, OV2_ERR_INVALID, "ov2_map_add_keyframe_px: null pixels");
    return add_keyframe_impl(m, kfid, Twc, n, lmid, unpx, runpx, is_stereo, scale, px, desc, has_desc);
}

extern "C" ov2_status ov2_map_set_landmarks(ov2_map *m, int n, const int32_t *lmid, const double *xyz, const uint8_t *state)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (n < 0 || (n && (!lmid || !state))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_landmarks: null argument");
    if (!n) return OV2_OK;
    int top_lm = -1;
    for (int i = 0; i < n; ++i) {
        if (lmid[i] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative lmid %d", lmid[i]);
        top_lm = std::max(top_lm, lmid[i]);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    {
        const ov2_status gs = ensure_capacity(m, 0, top_lm + 1, 0);
        if (gs != OV2_OK) return gs;
    }
    stager S{c};
    ov2_status s = S.begin((size_t)n * (sizeof(int) + 3 * sizeof(double) + 1) + 256);
    if (s != OV2_OK) return s;
    const int *dl = S.put(lmid, n);
    const double *dx = S.put(xyz, 3 * (size_t)n);
    const unsigned char *dst = S.put(state, n);
    if ((s = S.flush()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, map_set_lm_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dl, dx, dst, m->lm_xyz, m->lm_state);
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_map_set_poses(ov2_map *m, int n, const int32_t *kfid, const double *Twc)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (n < 0 || (n && (!kfid || !Twc))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_poses: null argument");
    if (!n) return OV2_OK;
    for (int i = 0; i < n; ++i)
        if (kfid[i] < 0 || kfid[i] >= m->max_kf) return ov2_set_err(c, OV2_ERR_INVALID, "kfid %d outside the map capacity", kfid[i]);
    OV2_HIP(c, hipSetDevice(c->device));
    stager S{c};
    ov2_status s = S.begin((size_t)n * (sizeof(int) + 7 * sizeof(double)) + 256);
    if (s != OV2_OK) return s;
    const int *dk = S.put(kfid, n);
    const double *dT = S.put(Twc, 7 * (size_t)n);
    if ((s = S.flush()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, map_set_pose_kernel, dim3((7 * n + 255) / 256), dim3(256), 0, c->stream, n, dk, dT, m->kf_pose);
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

static ov2_status edit_obs(ov2_map *m, int n, const int32_t *kfid, const int32_t *lmid, int mode, const uint8_t *st, const double *ruv)
{
    ov2_ctx *c = m->c;
    if (!n || !m->n_obs) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    stager S{c};
    ov2_status s = S.begin((size_t)n * (2 * sizeof(int) + 2 * sizeof(double) + 1) + 256);
    if (s != OV2_OK) return s;
    const int *dk = S.put(kfid, n);
    const int *dl = S.put(lmid, n);
    const unsigned char *ds = S.put(st, n);
    const double *dr = S.put(ruv, 2 * (size_t)n);
    if ((s = S.flush()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, map_edit_obs_kernel, dim3((m->n_obs + 255) / 256), dim3(256), 0, c->stream, m->n_obs, (const int *)m->obs_kf,
               (const int *)m->obs_lm, m->obs_flag, m->obs_ruv, n, dk, dl, mode, ds, dr);
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_map_remove_obs(ov2_map *m, int n, const int32_t *kfid, const int32_t *lmid)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    if (n < 0 || (n && (!kfid || !lmid))) return ov2_set_err(m->c, OV2_ERR_INVALID, "ov2_map_remove_obs: null argument");
    return edit_obs(m, n, kfid, lmid, 0, nullptr, nullptr);
}

extern "C" ov2_status ov2_map_set_obs_stereo(ov2_map *m, int n, const int32_t *kfid, const int32_t *lmid, const uint8_t *is_stereo,
                                             const double *runpx)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    if (n < 0 || (n && (!kfid || !lmid || !is_stereo || !runpx)))
        return ov2_set_err(m->c, OV2_ERR_INVALID, "ov2_map_set_obs_stereo: null argument");
    return edit_obs(m, n, kfid, lmid, 1, is_stereo, runpx);
}

extern "C" ov2_status ov2_map_set_obs_desc(ov2_map *m, int n, const int32_t *kfid, const int32_t *lmid, const float *px,
                                           const uint8_t *desc, const uint8_t *has_desc)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (!m->obs_hasdesc) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_obs_desc: the map has no match columns");
    if (n < 0 || (n && (!kfid || !lmid || !desc || !has_desc))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_obs_desc: null argument");
    if (!n || !m->n_obs) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    stager S{c};
    ov2_status s = S.begin((size_t)n * (2 * sizeof(int) + 2 * sizeof(float) + 33) + 256);
    if (s != OV2_OK) return s;
    const int *dk = S.put(kfid, n);
    const int *dl = S.put(lmid, n);
    const float *dp = S.put(px, 2 * (size_t)n);
    const uint8_t *dd = S.put(desc, 32 * (size_t)n), *dh = S.put(has_desc, (size_t)n);
    if ((s = S.flush()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, map_set_desc_kernel, dim3((m->n_obs + 255) / 256), dim3(256), 0, c->stream, m->n_obs, (const int *)m->obs_kf,
               (const int *)m->obs_lm, (const unsigned char *)m->obs_flag, reinterpret_cast<float2 *>(m->obs_px),
               reinterpret_cast<uint4 *>(m->obs_desc), m->obs_hasdesc, n, dk, dl, reinterpret_cast<const float2 *>(dp),
               reinterpret_cast<const uint4 *>(dd), dh);
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_map_remove_landmarks(ov2_map *m, int n, const int32_t *lmid)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (n < 0 || (n && !lmid)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_remove_landmarks: null argument");
    if (!n) return OV2_OK;
    // the landmark row dies; its observations stop counting through obs_live (their rows stay as tombstones)
    std::vector<uint8_t> zero((size_t)n, 0);
    return ov2_map_set_landmarks(m, n, lmid, nullptr, zero.data());
}

extern "C" ov2_status ov2_map_remove_keyframe(ov2_map *m, int kfid)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (kfid < 0 || kfid >= m->max_kf) return ov2_set_err(c, OV2_ERR_INVALID, "kfid %d outside the map capacity", kfid);
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipMemsetAsync(m->kf_state + kfid, 0, 1, c->stream));
    m->kf_alive_h[kfid] = 0;
    return ls_forget(m, kfid);
}

// ---- set-up of B maps: the whole chain of launches without a synchronisation, then one for the gathered headers ----
namespace {

ov2_status grow_out(ov2_map *m, size_t need)
{
    ov2_ctx *c = m->c;
    if (need <= m->out_cap) return OV2_OK;
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    if (m->out_dev) OV2_HIP(c, hipFree(m->out_dev));
    m->out_dev = nullptr; m->out_cap = 0;
    const size_t want = need + need / 2 + 4096;
    if (hipMalloc((void **)&m->out_dev, want) != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "flat problem block of %zu bytes", want);
    m->out_cap = want;
    return OV2_OK;
}

void fill_view(const ov2_map *m, unsigned char *base, ov2_local_ba_setup *out)
{
    const int *H = m->last_hdr;
    memset(out, 0, sizeof(*out));
    out->aborted = H[MH_ABORT];
    if (out->aborted) return;
    size_t off[FO_N];
    flat_layout((size_t)H[MH_NPOSE], (size_t)H[MH_NLM], (size_t)H[MH_NRES], (size_t)H[MH_NBAD], m->last_inv ? 1 : 3, off);
    const flat_out O = flat_ptrs(base, off);
    out->n_pose = H[MH_NPOSE]; out->n_lm = H[MH_NLM]; out->n_res = H[MH_NRES]; out->n_bad = H[MH_NBAD];
    out->pose_kfid = O.pose_kfid; out->pose_const = O.pose_const; out->pose = O.pose;
    out->lm_lmid = O.lm_lmid; out->lm = O.lm; out->lm_anchor_pose = O.lm_anchor_pose; out->lm_anchor_uv = O.lm_anchor_uv;
    out->res_type = O.res_type; out->res_pose = O.res_pose; out->res_lm = O.res_lm; out->res_uv = O.res_uv; out->res_sigma = O.res_sigma;
    out->bad_lmid = O.bad_lmid;
    out->res_outlier = base == m->out_dev ? O.res_out : nullptr;   // device form only
}

// enqueues the set-up chain for the maps of `sel` (indices into maps[]), fetches their headers (one synchronisation)
// lo != nullptr: the set-up of looseBA over the keyframes [lo[b], newkf[b]] (its own selection kernel, the rest of the chain as it is)
ov2_status setup_pass(ov2_ctx *c, const std::vector<int> &sel, ov2_map *const *maps, const int32_t *newkf, int nmin_cov, int nmin_cst,
                      int inv, const int32_t *lo)
{
    const int B = (int)sel.size();
    hipStream_t st = c->stream;
    job_table JT;
    ov2_status s = JT.begin(c, B);
    if (s != OV2_OK) return s;
    int nmax = 0, lmax = 0, kmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[sel[b]];
        if (!m->out_dev && (s = grow_out(m, 1u << 20)) != OV2_OK) return s;
        map_job j = job_of(m, newkf[sel[b]], -1);
        j.lb_lo = lo ? lo[sel[b]] : 0;
        JT.set(b, j);
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); kmax = std::max(kmax, m->max_kf);
        zmax = std::max(zmax, (unsigned)(m->zero_bytes / 16));
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gL((lmax + 255) / 256, B), gK((kmax + 255) / 256, B), one(1, B), b(256);
    const map_job *J = JT.dev;
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b, 0, st, J);
    OV2_LAUNCH(c, OV2_K_MAP, ms_count_kernel, gN, b, 0, st, J);
    if (lo) OV2_LAUNCH(c, OV2_K_MAP, ml_select_kernel, one, dim3(64), 0, st, J, nmin_cst);
    else {
        OV2_LAUNCH(c, OV2_K_MAP, ms_cov_kernel, gN, b, 0, st, J);
        OV2_LAUNCH(c, OV2_K_MAP, ms_select_kernel, one, dim3(64), 0, st, J, nmin_cov);
    }
    OV2_LAUNCH(c, OV2_K_MAP, ms_local_lm_kernel, gN, b, 0, st, J);
    OV2_LAUNCH(c, OV2_K_MAP, ms_observers_kernel, gN, b, 0, st, J);
    OV2_LAUNCH(c, OV2_K_MAP, ms_poses_kernel, one, dim3(1024), 0, st, J, nmin_cst);
    OV2_LAUNCH(c, OV2_K_MAP, ms_lm_flags_kernel, gL, b, 0, st, J, inv);
    // one 64-bit scan numbers the landmarks (low word) and the bad list (high word); its total lands on NLM | NBAD
    if ((s = exclusive_scan<unsigned long long>(c, JT, SC_LM, lmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, ms_res_count_kernel, gN, b, 0, st, J, inv);
    if ((s = exclusive_scan<int>(c, JT, SC_RES, nmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, me_all_kernel, dim3(gK.x + gL.x + gN.x, B), b, 0, st, J, (int)gK.x, (int)gL.x, inv);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b2 = 0; b2 < B; ++b2) {
        ov2_map *m = maps[sel[b2]];
        memcpy(m->last_hdr, JT.hdr_host + (size_t)b2 * MH_N, MH_N * sizeof(int));
        m->last_newkf = newkf[sel[b2]]; m->last_inv = inv; m->last_valid = 1;
        m->last_n_obs = m->n_obs; m->last_updated = 0; m->last_kind = lo ? 1 : 0;
        m->live_rows = m->last_hdr[MH_NLIVE]; m->live_known = 1;
    }
    return OV2_OK;
}

// the refusals the batch entry points share, one per call so that every entry point keeps its own order of checks
ov2_status batch_map_ok(ov2_ctx *c, const ov2_map *m, int b)
{
    if (!m || m->c != c) return ov2_set_err(c, OV2_ERR_INVALID, "map %d of the batch is null or belongs to another context", b);
    return OV2_OK;
}

ov2_status batch_map_once(ov2_ctx *c, ov2_map *const *maps, int b)
{
    for (int q = 0; q < b; ++q)
        if (maps[q] == maps[b]) return ov2_set_err(c, OV2_ERR_INVALID, "map %d appears twice in the batch", b);
    return OV2_OK;
}

ov2_status batch_kf_alive(ov2_ctx *c, const ov2_map *m, int kfid, int b)
{
    if (kfid < 0 || kfid >= m->max_kf || !m->kf_alive_h[kfid])
        return ov2_set_err(c, OV2_ERR_INVALID, "keyframe %d is not alive in map %d", kfid, b);
    return OV2_OK;
}

// a stage's own header and cleared block stand where the kernels shared with the set-up look for them
void stage_block(map_job &j, unsigned char *blk, size_t bytes)
{
    j.hdr = reinterpret_cast<int *>(blk); j.zero_blk = blk; j.zero_vec16 = (unsigned)(bytes / 16);
}

ov2_status setup_batch_impl(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, int nmin_cov, int nmin_cst, int inv,
                            const double *calib_l, bool squeeze_first, const int32_t *lo = nullptr)
{
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if (newkf[b] < 0 || newkf[b] >= m->max_kf) return ov2_set_err(c, OV2_ERR_INVALID, "kfid %d outside the capacity of map %d", newkf[b], b);
        if (lo && (s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        if (lo && lo[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the range starts at keyframe %d", b, lo[b]);
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
    }
    for (int b = 0; b < B; ++b) {   // nothing of a refused call reaches a map (the local set-up's intrinsics included)
        ov2_map *m = maps[b];
        m->have_K = calib_l != nullptr;
        for (int k = 0; k < 4; ++k) m->last_K[k] = calib_l ? calib_l[4 * b + k] : 0.0;
    }
    OV2_HIP(c, hipSetDevice(c->device));
    if (squeeze_first)   // the batched form squeezes a mostly dead table BEFORE the chain: its update stage needs the row indices after it
        for (int b = 0; b < B; ++b) {
            ov2_map *m = maps[b];
            if (m->live_known && squeeze_due(m, m->live_rows)) {
                const ov2_status cs = compact_obs(m);
                if (cs != OV2_OK) return cs;
            }
        }
    std::vector<int> sel((size_t)B);
    for (int b = 0; b < B; ++b) sel[b] = b;
    for (int pass = 0; pass < 3 && !sel.empty(); ++pass) {
        if ((s = setup_pass(c, sel, maps, newkf, nmin_cov, nmin_cst, inv, lo)) != OV2_OK) return s;
        // a flat problem that did not fit its block: grow the block, run that map again (first calls / growing windows only)
        std::vector<int> again;
        for (int b : sel) {
            ov2_map *m = maps[b];
            if (!m->last_hdr[MH_OVER]) continue;
            if ((s = grow_out(m, (size_t)m->last_hdr[MH_NEED16] << 4)) != OV2_OK) return s;
            again.push_back(b);
        }
        sel.swap(again);
    }
    if (!sel.empty()) return ov2_set_err(c, OV2_ERR_NOMEM, "flat problem blocks kept overflowing");
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_map_local_ba_setup_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, int nmin_covscore,
                                                   int nmin_cst_kfs, int inv_depth, const double *calib_l, ov2_local_ba_setup *dev)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !dev) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_local_ba_setup_batch: null argument");
    const ov2_status s = setup_batch_impl(c, B, maps, newkf, nmin_covscore, nmin_cst_kfs, inv_depth ? 1 : 0, calib_l, true);
    if (s != OV2_OK) return s;
    for (int b = 0; b < B; ++b) fill_view(maps[b], maps[b]->out_dev, &dev[b]);
    return OV2_OK;
}

extern "C" ov2_status ov2_map_local_ba_setup(ov2_map *m, int newkf, int nmin_covscore, int nmin_cst_kfs, int inv_depth,
                                             const double *calib_l, ov2_local_ba_setup *out)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (!out) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_local_ba_setup: null output");
    memset(out, 0, sizeof(*out));
    const int32_t nk = newkf;
    ov2_status s = setup_batch_impl(c, 1, &m, &nk, nmin_covscore, nmin_cst_kfs, inv_depth ? 1 : 0, calib_l, false);
    if (s != OV2_OK) return s;
    const int *H = m->last_hdr;
    // mostly tombstones left: squeeze the table once this set-up has read it (amortised like a growth)
    const bool squeeze = squeeze_due(m, H[MH_NLIVE]);
    if (H[MH_ABORT]) { out->aborted = 1; return squeeze ? compact_obs(m) : OV2_OK; }
    // the host form: the arrays of the flat problem into the pinned mirror (second synchronisation)
    size_t off[FO_N];
    flat_layout((size_t)H[MH_NPOSE], (size_t)H[MH_NLM], (size_t)H[MH_NRES], (size_t)H[MH_NBAD], inv_depth ? 1 : 3, off);
    const size_t bytes = off[FO_HOST_END];
    if (bytes > m->out_host_cap) {
        if (m->out_host) OV2_HIP(c, hipHostFree(m->out_host));
        m->out_host = nullptr; m->out_host_cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc((void **)&m->out_host, want, hipHostMallocDefault) != hipSuccess)
            return ov2_set_err(c, OV2_ERR_NOMEM, "pinned flat problem of %zu bytes", want);
        m->out_host_cap = want;
    }
    if (bytes) OV2_HIP(c, hipMemcpyAsync(m->out_host, m->out_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    fill_view(m, m->out_host, out);
    return squeeze ? compact_obs(m) : OV2_OK;
}

// The same flat problem, where the set-up left it on the device (ov2_ba_solve_batch_dev takes these pointers as they are)
extern "C" ov2_status ov2_map_setup_device_view(const ov2_map *m, const ov2_local_ba_setup *host, ov2_local_ba_setup *dev)
{
    if (!m || !host || !dev) return OV2_ERR_INVALID;
    if (host->aborted) { *dev = *host; return OV2_OK; }
    const unsigned char *q = (const unsigned char *)host->pose_kfid;
    if (!m->out_dev || !(m->out_host && q >= m->out_host && q < m->out_host + m->out_host_cap)) return OV2_ERR_INVALID;   // not the arrays of this map's last set-up
    if (host->n_pose != m->last_hdr[MH_NPOSE] || host->n_lm != m->last_hdr[MH_NLM] || host->n_res != m->last_hdr[MH_NRES])
        return OV2_ERR_INVALID;
    fill_view(m, m->out_dev, dev);
    return OV2_OK;
}

// ---- update stage of B maps --------------------------------------------------------------------------------------
extern "C" ov2_status ov2_map_local_ba_update_batch(ov2_ctx *c, int B, ov2_map *const *maps, const uint8_t *const *d_outlier,
                                                    const int32_t *cur_kfid, ov2_local_ba_update *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_local_ba_update_batch: null argument");
    int inv = -1;
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if (!m->last_valid)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: no set-up to update from (none ran, or the tables grew / were squeezed "
                               "/ restored since)", b);
        if (m->last_updated)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the update stage of its last set-up has already run", b);
        if (m->last_kind != 0)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: its last set-up is looseBA's (ov2_map_loose_ba_update_batch updates from it)", b);
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        if (inv < 0) inv = m->last_inv;
        if (m->last_inv != inv) return ov2_set_err(c, OV2_ERR_INVALID, "the maps of a batch must share one landmark parametrisation (map %d)", b);
        if (inv && !m->have_K && !m->last_hdr[MH_ABORT])
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the inverse-depth update needs the left intrinsics (calib_l of the set-up)", b);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    job_table JT;
    if ((s = JT.begin(c, B)) != OV2_OK) return s;
    int nset = 0, nnow = 0, pmax = 0, lmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        map_job j = job_of(m, m->last_newkf, cur_kfid ? cur_kfid[b] : -1);
        j.outlier = d_outlier ? d_outlier[b] : nullptr;
        j.last_n_obs = m->last_n_obs;
        JT.set(b, j);
        if (m->last_hdr[MH_ABORT]) continue;
        nset = std::max(nset, m->last_n_obs); nnow = std::max(nnow, m->n_obs); pmax = std::max(pmax, m->last_hdr[MH_NPOSE]);
        lmax = std::max(lmax, m->last_hdr[MH_NLM] + m->last_hdr[MH_NBAD]);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    // rows of the set-up (pass 1) vs rows now (pass 1b: appended rows are observers too)
    const int gN = (nset + 255) / 256, gNow = (nnow + 255) / 256;
    const dim3 b256(256);
    const int gP = (pmax + 255) / 256, gLM = (lmax + 255) / 256;
    if (gN + gLM > 0) OV2_LAUNCH(c, OV2_K_MAP, mu_obs_kernel, dim3(gN + gLM, B), b256, 0, st, JT.dev, gN, inv);
    if (gNow > 0 && gLM > 0) OV2_LAUNCH(c, OV2_K_MAP, mu_recount_kernel, dim3(gNow, B), b256, 0, st, JT.dev);
    if (gP + gLM > 0) OV2_LAUNCH(c, OV2_K_MAP, mu_apply_kernel, dim3(gP + gLM, B), b256, 0, st, JT.dev, gP, inv);
    for (int b = 0; b < B; ++b) maps[b]->last_updated = 1;
    if (!out) return OV2_OK;   // asynchronous: the caller did not ask for what to replay
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        const int *H = JT.hdr_host + (size_t)b * MH_N;
        memset(&out[b], 0, sizeof(out[b]));
        if (m->last_hdr[MH_ABORT]) continue;
        size_t off[FO_N];
        flat_layout((size_t)m->last_hdr[MH_NPOSE], (size_t)m->last_hdr[MH_NLM], (size_t)m->last_hdr[MH_NRES], (size_t)m->last_hdr[MH_NBAD],
                    inv ? 1 : 3, off);
        const flat_out O = flat_ptrs(m->out_dev, off);
        out[b].n_removed_lm = H[MH_NRM_LM]; out[b].n_removed_obs = H[MH_NRM_OBS]; out[b].n_stereo_off = H[MH_NST_OFF];
        out[b].removed_lmid = O.rm_lm; out[b].removed_obs = (const int32_t *)O.rm_obs; out[b].stereo_off = (const int32_t *)O.st_off;
    }
    return OV2_OK;
}

// ---- looseBA of B maps: the set-up chain with its own selection, the update in seven launches whatever B ----------------
extern "C" ov2_status ov2_map_loose_ba_setup_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *inikfid, const int32_t *nkfid,
                                                   int nmin_cst_kfs, int inv_depth, const double *calib_l, ov2_local_ba_setup *dev)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !inikfid || !nkfid || !dev) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_loose_ba_setup_batch: null argument");
    const ov2_status s = setup_batch_impl(c, B, maps, nkfid, 0, nmin_cst_kfs, inv_depth ? 1 : 0, calib_l, true, inikfid);
    if (s != OV2_OK) return s;
    for (int b = 0; b < B; ++b) fill_view(maps[b], maps[b]->out_dev, &dev[b]);
    return OV2_OK;
}

extern "C" ov2_status ov2_map_loose_ba_update_batch(ov2_ctx *c, int B, ov2_map *const *maps, const uint8_t *const *d_outlier,
                                                    const int32_t *cur_kfid, ov2_local_ba_update *lists, ov2_map_loose_ba *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_loose_ba_update_batch: null argument");
    int inv = -1;
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if (!m->last_valid)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: no set-up to update from (none ran, or the tables grew / were squeezed "
                               "/ restored / edited by another stage since)", b);
        if (m->last_updated)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the update stage of its last set-up has already run", b);
        if (m->last_kind != 1)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: its last set-up is localBA's (ov2_map_local_ba_update_batch updates from it)", b);
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        if (inv < 0) inv = m->last_inv;
        if (m->last_inv != inv) return ov2_set_err(c, OV2_ERR_INVALID, "the maps of a batch must share one landmark parametrisation (map %d)", b);
        if (inv && !m->have_K && m->last_hdr[MH_NRES])
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the inverse-depth update needs the left intrinsics (calib_l of the set-up)", b);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    job_table JT;
    if ((s = JT.begin(c, B, LB_EXTRA_INTS)) != OV2_OK) return s;
    int nset = 0, nnow = 0, lmax = 0, kmax = 0, lmmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        map_job j = job_of(m, m->last_newkf, cur_kfid ? cur_kfid[b] : -1);
        j.outlier = d_outlier ? d_outlier[b] : nullptr;
        j.last_n_obs = m->last_n_obs;
        j.lb_on = m->last_hdr[MH_NRES] > 0;   // a problem without a residual block changes nothing (:1272)
        if (!j.lb_on) { j.outlier = nullptr; j.last_n_obs = 0; }
        JT.set(b, j);
        JT.host[b].lb_cnt = JT.host[b].hdr_out + MH_N;
        JT.host[b].lb_tmp = (double *)(JT.host[b].hdr_out + MH_N + LB_N);
        if (!j.lb_on) continue;
        nset = std::max(nset, m->last_n_obs); nnow = std::max(nnow, m->n_obs); kmax = std::max(kmax, m->max_kf);
        lmax = std::max(lmax, m->last_hdr[MH_NLM] + m->last_hdr[MH_NBAD]); lmmax = std::max(lmmax, m->max_lm);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 b256(256);
    const int gN = (nset + 255) / 256, gNow = (nnow + 255) / 256, gLM = (lmax + 255) / 256;
    const dim3 gL((std::max(lmmax, 1) + 255) / 256, B), gK((std::max(kmax, 1) + 255) / 256, B);
    OV2_LAUNCH(c, OV2_K_MAP, ml_clear_kernel, gL, b256, 0, st, JT.dev, inv);
    if (gNow > 0) {
        OV2_LAUNCH(c, OV2_K_MAP, ml_observers_kernel, dim3(gNow, B), b256, 0, st, JT.dev, inv);
        OV2_LAUNCH(c, OV2_K_MAP, ml_landmarks_kernel, gL, b256, 0, st, JT.dev, inv);
        OV2_LAUNCH(c, OV2_K_MAP, ml_poses_kernel, gK, b256, 0, st, JT.dev, inv);
        if (gN + gLM > 0) OV2_LAUNCH(c, OV2_K_MAP, mu_obs_kernel, dim3(gN + gLM, B), b256, 0, st, JT.dev, gN, inv);
        if (gLM > 0) {
            OV2_LAUNCH(c, OV2_K_MAP, mu_recount_kernel, dim3(gNow, B), b256, 0, st, JT.dev);
            OV2_LAUNCH(c, OV2_K_MAP, ml_cull_kernel, dim3(gLM, B), b256, 0, st, JT.dev, inv);
        }
    }
    for (int b = 0; b < B; ++b) maps[b]->last_updated = 1;
    if (!out && !lists) return OV2_OK;   // asynchronous: the caller did not ask for anything
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        const int *H = JT.hdr_host + (size_t)b * JT.stride, *C = H + MH_N;
        const bool ran = m->last_hdr[MH_NRES] > 0;
        if (lists) {
            memset(&lists[b], 0, sizeof(lists[b]));
            if (ran) {
                size_t off[FO_N];
                flat_layout((size_t)m->last_hdr[MH_NPOSE], (size_t)m->last_hdr[MH_NLM], (size_t)m->last_hdr[MH_NRES],
                            (size_t)m->last_hdr[MH_NBAD], inv ? 1 : 3, off);
                const flat_out O = flat_ptrs(m->out_dev, off);
                lists[b].n_removed_lm = H[MH_NRM_LM]; lists[b].n_removed_obs = H[MH_NRM_OBS]; lists[b].n_stereo_off = H[MH_NST_OFF];
                lists[b].removed_lmid = O.rm_lm; lists[b].removed_obs = (const int32_t *)O.rm_obs; lists[b].stereo_off = (const int32_t *)O.st_off;
            }
        }
        if (!out) continue;
        ov2_map_loose_ba &r = out[b];
        memset(&r, 0, sizeof(r));
        r.termination = OV2_BA_TERM_SKIPPED;
        if (!ran) continue;
        r.ran = 1;
        r.n_pose = H[MH_NPOSE]; r.n_free_pose = C[LB_FREE]; r.n_lm = H[MH_NLM]; r.n_res = H[MH_NRES]; r.n_bad = C[LB_BAD];
        r.n_flagged_left = C[LB_FLAG_L]; r.n_flagged_right = C[LB_FLAG_R]; r.n_removed_obs = H[MH_NRM_OBS]; r.n_stereo_off = H[MH_NST_OFF];
        r.n_removed_lm = H[MH_NRM_LM]; r.n_written = C[LB_WRITTEN]; r.n_propagated = C[LB_PROP]; r.n_kf_younger = C[LB_YOUNGER];
        memcpy(r.T_corr, (const double *)(C + LB_N) + 14, 7 * sizeof(double));
    }
    return OV2_OK;
}

extern "C" void ov2_ba_loose_options(ov2_ba_options *o, float robust_mono_th, int robust)
{
    ov2_ba_default_options(o, robust_mono_th);
    if (!robust) o->huber_delta = 0.0;
    o->max_iters = 5; o->function_tolerance = 1e-4;   // src/optimizer.cpp:1298-1299
    o->l2_refine = 0;                                 // one solve; the flags only pick what is removed
}

extern "C" ov2_status ov2_map_loose_ba_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *inikfid, const int32_t *nkfid,
                                             const ov2_map_sba_cam *cam, int stereo, int inv_depth, const ov2_ba_options *o,
                                             const int32_t *cur_kfid, ov2_local_ba_update *lists, ov2_map_loose_ba *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !inikfid || !nkfid || !cam || !o) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_loose_ba_batch: null argument");
    std::vector<double> K((size_t)B * 4);
    for (int b = 0; b < B; ++b) memcpy(&K[4 * (size_t)b], cam[b].calib_l, 4 * sizeof(double));
    std::vector<ov2_local_ba_setup> V((size_t)B);
    ov2_status s = ov2_map_loose_ba_setup_batch(c, B, maps, inikfid, nkfid, stereo ? 1 : 2, inv_depth, K.data(), V.data());
    if (s != OV2_OK) return s;
    std::vector<ov2_ba_problem> P;
    std::vector<ov2_ba_result> R;
    std::vector<int> who;
    std::vector<const uint8_t *> flags((size_t)B, nullptr);
    for (int b = 0; b < B; ++b) {
        const ov2_local_ba_setup &v = V[b];
        if (v.n_res <= 0) continue;
        ov2_ba_problem p;
        memset(&p, 0, sizeof(p));
        memcpy(p.calib_l, cam[b].calib_l, sizeof(p.calib_l)); memcpy(p.calib_r, cam[b].calib_r, sizeof(p.calib_r));
        memcpy(p.T_rl, cam[b].T_rl, sizeof(p.T_rl));
        p.inv_depth = inv_depth ? 1 : 0;
        p.n_pose = v.n_pose; p.pose = v.pose; p.pose_const = v.pose_const;
        p.n_lm = v.n_lm; p.lm = v.lm; p.lm_anchor_pose = v.lm_anchor_pose; p.lm_anchor_uv = v.lm_anchor_uv;
        p.n_res = v.n_res; p.res_type = v.res_type; p.res_pose = v.res_pose; p.res_lm = v.res_lm; p.res_uv = v.res_uv; p.res_sigma = v.res_sigma;
        ov2_ba_result r;
        memset(&r, 0, sizeof(r));
        r.outlier = v.res_outlier;
        P.push_back(p); R.push_back(r); who.push_back(b);
        flags[b] = v.res_outlier;
    }
    if (!P.empty() && (s = ov2_ba_solve_batch_dev(c, (int)P.size(), P.data(), o, R.data())) != OV2_OK) return s;
    if ((s = ov2_map_loose_ba_update_batch(c, B, maps, flags.data(), cur_kfid, lists, out)) != OV2_OK) return s;
    if (out)
        for (size_t w = 0; w < who.size(); ++w) {
            ov2_map_loose_ba &r = out[who[w]];
            r.termination = R[w].termination; r.n_outliers_pass1 = R[w].n_outliers_pass1; r.n_log = R[w].n_log;
            r.initial_cost = R[w].initial_cost; r.final_cost = R[w].final_cost;
            memcpy(r.log, R[w].log, sizeof(r.log));
        }
    return OV2_OK;
}

// ---- temporal triangulation of B maps: four launches, no synchronisation unless the lists are asked for -------------
extern "C" ov2_status ov2_map_triangulate_temporal_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                         const double *calib_l, int stereo, float max_reproj_err, ov2_map_temporal *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !calib_l) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_triangulate_temporal_batch: null argument");
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    job_table JT;
    if ((s = JT.begin(c, B)) != OV2_OK) return s;
    int nmax = 0, lmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        map_job j = job_of(m, newkf[b], -1);
        stage_block(j, m->tt_zero, m->tt_zero_bytes);
        j.tt_nobs = m->tt_nobs; j.tt_old = m->tt_old; j.tt_nrow = m->tt_nrow;
        j.tt_arow = m->tt_int; j.tt_good_lmid = m->tt_int + m->max_lm; j.tt_rm_lmid = m->tt_int + 2 * (size_t)m->max_lm;
        j.tt_good_wpt = m->tt_dbl; j.tt_good_inv = m->tt_dbl + 3 * (size_t)m->max_lm;
        for (int k = 0; k < 4; ++k) j.K[k] = calib_l[4 * b + k];
        JT.set(b, j);
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); zmax = std::max(zmax, j.zero_vec16);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gL((lmax + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mt_observers_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mt_rows_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mt_tri_kernel, gL, b256, 0, st, JT.dev, stereo ? 1 : 0, max_reproj_err);
    if (!out) return OV2_OK;   // asynchronous: the caller did not ask for what to replay
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        const int *H = JT.hdr_host + (size_t)b * MH_N;
        out[b].n_selected = H[TH_SELECTED]; out[b].n_candidates = H[TH_CANDIDATES]; out[b].n_good = H[TH_GOOD]; out[b].n_removed = H[TH_REMOVED];
        out[b].good_lmid = m->tt_int + m->max_lm; out[b].removed_lmid = m->tt_int + 2 * (size_t)m->max_lm;
        out[b].good_wpt = m->tt_dbl; out[b].good_invdepth = m->tt_dbl + 3 * (size_t)m->max_lm;
    }
    return OV2_OK;
}

// ---- the stereo matcher's verdicts onto the rows of B maps: three launches, no synchronisation ---------------------------
extern "C" ov2_status ov2_map_set_obs_stereo_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *kfid, const int32_t *n,
                                                       const int32_t *const *d_lmid, const uint8_t *const *d_status,
                                                       const float *const *d_rxy, const ov2_cam_model *right_cam)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !kfid || !n || !d_lmid || !d_status || !d_rxy)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_set_obs_stereo_batch_dev: null argument");
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_kf_alive(c, m, kfid[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        if (n[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: a list of %d entries", b, n[b]);
        if (n[b] > 0 && (!d_lmid[b] || !d_status[b] || !d_rxy[b])) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: a null list of %d entries", b, n[b]);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    job_table JT;
    if ((s = JT.begin(c, B)) != OV2_OK) return s;
    int nmax = 0, emax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        map_job j = job_of(m, kfid[b], -1);
        stage_block(j, m->ts_zero, m->ts_zero_bytes);
        j.ts_mark = m->ts_mark;
        j.si_n = n[b]; j.si_lmid = d_lmid[b]; j.si_status = d_status[b]; j.si_rxy = d_rxy[b];
        j.si_cam = ov2_cam_normalised(right_cam ? right_cam + b : nullptr);
        JT.set(b, j);
        nmax = std::max(nmax, m->n_obs); emax = std::max(emax, n[b]); zmax = std::max(zmax, j.zero_vec16);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gE((std::max(emax, 1) + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, si_scatter_kernel, gE, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, si_rows_kernel, gN, b256, 0, st, JT.dev);
    return OV2_OK;
}

// ---- stereo triangulation of B maps: two launches, no synchronisation unless the lists are asked for ---------------------
extern "C" ov2_status ov2_map_triangulate_stereo_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                       const ov2_stereo_rig *rig, float max_reproj_err, ov2_map_stereo_tri *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !rig) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_triangulate_stereo_batch: null argument");
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    job_table JT;
    if ((s = JT.begin(c, B)) != OV2_OK) return s;
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        map_job j = job_of(m, newkf[b], -1);
        stage_block(j, m->ts_zero, MH_N * sizeof(int));   // the header alone: the intake's marks are of no use here
        j.ts_good_lmid = m->ts_int; j.ts_dem_lmid = m->ts_int + m->max_lm; j.ts_why = m->ts_why;
        j.ts_good_wpt = m->ts_dbl; j.ts_good_inv = m->ts_dbl + 3 * (size_t)m->max_lm;
        for (int k = 0; k < 4; ++k) { j.K[k] = rig[b].Kl[k]; j.st_Kr[k] = rig[b].Kr[k]; }
        for (int k = 0; k < 7; ++k) j.st_Tlr[k] = rig[b].Tlr[k];
        j.st_rect = rig[b].rectified ? 1 : 0;
        JT.set(b, j);
        nmax = std::max(nmax, m->n_obs);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(1, B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mst_tri_kernel, gN, b256, 0, st, JT.dev, max_reproj_err);
    if (!out) return OV2_OK;   // asynchronous: the caller did not ask for what to replay
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        const int *H = JT.hdr_host + (size_t)b * MH_N;
        out[b].n_selected = H[SH_SELECTED]; out[b].n_good = std::min(H[SH_GOOD], m->max_lm); out[b].n_demoted = std::min(H[SH_DEMOTED], m->max_lm);
        out[b].good_lmid = m->ts_int; out[b].good_wpt = m->ts_dbl; out[b].good_invdepth = m->ts_dbl + 3 * (size_t)m->max_lm;
        out[b].demoted_lmid = m->ts_int + m->max_lm; out[b].demoted_why = m->ts_why;
    }
    return OV2_OK;
}

// ---- keyframe culling of B maps: seven launches whatever B, one synchronisation for the headers and removed lists ---
extern "C" ov2_status ov2_map_filter_keyframes_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, int nmin_covscore,
                                                     float kf_filtering_ratio, ov2_map_filter *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !out) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_filter_keyframes_batch: null argument");
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
    }
    memset(out, 0, (size_t)B * sizeof(*out));
    // src/estimator.cpp:103-109: the reference's "off" value of the ratio, and no culling before keyframe 20
    int n_active = 0, nmax = 0, kmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b)
        if (!(kf_filtering_ratio >= 1.f) && newkf[b] >= 20) { ++n_active; kmax = std::max(kmax, maps[b]->max_kf); }
    if (!n_active) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    for (int b = 0; b < B; ++b) {   // the pinned list of the map follows its keyframe capacity
        ov2_map *m = maps[b];
        if (m->fl_removed_cap >= m->max_kf) continue;
        if (m->fl_removed_h) OV2_HIP(c, hipHostFree(m->fl_removed_h));
        m->fl_removed_h = nullptr; m->fl_removed_cap = 0;
        if (hipHostMalloc((void **)&m->fl_removed_h, (size_t)m->max_kf * sizeof(int), hipHostMallocDefault) != hipSuccess)
            return ov2_set_err(c, OV2_ERR_NOMEM, "pinned keyframe list of %d entries", m->max_kf);
        m->fl_removed_cap = m->max_kf;
    }
    job_table JT;
    if ((s = JT.begin(c, B, kmax)) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        map_job j = job_of(m, newkf[b], -1);
        j.fl_active = newkf[b] >= 20;
        stage_block(j, m->fl_zero, j.fl_active ? m->fl_zero_bytes : 0);
        j.fl_nobs = m->fl_nobs; j.fl_cov = m->fl_cov; j.fl_n3d = m->fl_n3d; j.fl_cnt = m->fl_cnt; j.fl_fill = m->fl_fill;
        j.fl_new = m->fl_new; j.fl_start = m->fl_start; j.fl_rows = m->fl_rows; j.fl_unset = m->fl_unset;
        JT.set(b, j);
        if (j.fl_active) { nmax = std::max(nmax, m->n_obs); zmax = std::max(zmax, j.zero_vec16); }
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mf_count_kernel, gN, b256, 0, st, JT.dev);
    if ((s = exclusive_scan<int>(c, JT, SC_KF, kmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mf_index_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mf_walk_kernel, dim3(1, B), dim3(MF_THREADS), 0, st, JT.dev, nmin_covscore, kf_filtering_ratio, kmax);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        if (newkf[b] < 20) continue;
        const int *H = JT.hdr_host + (size_t)b * JT.stride;
        out[b].n_candidates = H[FH_CANDIDATES]; out[b].n_removed = H[FH_REMOVED]; out[b].n_few3d = H[FH_FEW3D]; out[b].n_unset3d = H[FH_UNSET3D];
        out[b].removed_kfid = m->fl_removed_h; out[b].unset3d_lmid = m->fl_unset;
        for (int i = 0; i < H[FH_REMOVED]; ++i) {
            const int k = H[MH_N + i];
            m->fl_removed_h[i] = k;
            m->kf_alive_h[k] = 0;
            if ((s = ls_forget(m, k)) != OV2_OK) return s;   // its local id set goes with it
        }
        m->last_valid = 0;   // its tables changed under the last set-up: no update stage from it any more
    }
    return OV2_OK;
}

// ---- local-map selection of B maps: nine launches whatever B, one synchronisation for the headers and the lists ----------
extern "C" ov2_status ov2_map_local_ids_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, int extend, int nmax_local,
                                              ov2_map_local_ids *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !out) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_local_ids_batch: null argument");
    if (nmax_local < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_local_ids_batch: nmax_local %d", nmax_local);
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if (!m->ls_on) return ov2_set_err(c, OV2_ERR_INVALID, "map %d of the batch has no local sets", b);
        if ((s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
    }
    memset(out, 0, (size_t)B * sizeof(*out));
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // The host knows every count: the new set is a subset of S + old + extension, all distinct ids below max_lm.  That many
    // entries are reserved in the pool and in the gathered copy before anything is enqueued.
    int nmax = 0, lmax = 0, kmax = 0, room_max = 0; unsigned zmax = 0;
    std::vector<int> room((size_t)B);
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        int top = 0;
        for (int k = 0; k < m->max_kf; ++k) top = std::max(top, m->ls_count_h[k]);
        room[b] = (int)std::min<long long>(m->max_lm, (long long)m->n_obs + m->ls_count_h[newkf[b]] + top);
        if ((s = ls_reserve(m, room[b])) != OV2_OK) return s;
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); kmax = std::max(kmax, m->max_kf);
        room_max = std::max(room_max, room[b]);
        zmax = std::max(zmax, (unsigned)(m->ls_zero_bytes / 16));
    }
    for (int b = 0; b < B; ++b) {   // the pinned lists of the map: two covisibility lists and the ids
        ov2_map *m = maps[b];
        const int need = 2 * m->max_kf + room[b];
        if (m->ls_out_cap >= need) continue;
        if (m->ls_out_h) OV2_HIP(c, hipHostFree(m->ls_out_h));
        m->ls_out_h = nullptr; m->ls_out_cap = 0;
        if (hipHostMalloc((void **)&m->ls_out_h, (size_t)need * sizeof(int), hipHostMallocDefault) != hipSuccess)
            return ov2_set_err(c, OV2_ERR_NOMEM, "pinned local-map lists of %d entries", need);
        m->ls_out_cap = need;
    }
    job_table JT;
    if ((s = JT.begin(c, B, 2 * kmax + room_max)) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        map_job j = job_of(m, newkf[b], -1);
        stage_block(j, m->ls_zero, m->ls_zero_bytes);
        j.ls_on = 1; j.ls_extend = extend != 0; j.ls_nmax = nmax_local; j.ls_kcap = kmax; j.ls_room = room[b];
        j.ls_pool_off = m->ls_pool_used;
        j.ls_cov = m->ls_cov; j.ls_mark = m->ls_mark; j.ls_obs = m->ls_obs; j.ls_pos = m->ls_pos;
        j.ls_pool = m->ls_pool; j.ls_start = m->ls_start; j.ls_count = m->ls_count;
        JT.set(b, j);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gL((lmax + 255) / 256, B), one(1, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, li_obs_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, li_cov_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, li_fresh_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, li_lists_kernel, one, dim3(1024), 0, st, JT.dev);
    if ((s = exclusive_scan<int>(c, JT, SC_LS, lmax)) != OV2_OK) return s;
    // lmax >= 1 (ov2_map_create refuses a capacity of 0 and the tables only grow): the grid is never empty, and its first
    // thread hands the header over whatever the marks hold
    OV2_LAUNCH(c, OV2_K_MAP, li_emit_kernel, gL, b256, 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        const int *H = JT.hdr_host + (size_t)b * JT.stride;
        const int k = newkf[b], n_cov = H[LH_NCOV], n_local = H[LH_NLOCAL];
        if (n_local > room[b] || n_cov > kmax) return ov2_set_err(c, OV2_ERR_HIP, "map %d: a local-map list outgrew its reserve", b);
        int *cov_kfid = m->ls_out_h, *cov_score = cov_kfid + m->max_kf, *lmid = cov_score + m->max_kf;
        memcpy(cov_kfid, H + MH_N, (size_t)n_cov * sizeof(int));
        memcpy(cov_score, H + MH_N + kmax, (size_t)n_cov * sizeof(int));
        memcpy(lmid, H + MH_N + 2 * kmax, (size_t)n_local * sizeof(int));
        out[b].n_cov = n_cov; out[b].oldest_cov = H[LH_OLDEST]; out[b].n_fresh = H[LH_NFRESH]; out[b].n_local = n_local;
        out[b].swapped = H[LH_SWAPPED]; out[b].extended = H[LH_EXTENDED];
        out[b].cov_kfid = cov_kfid; out[b].cov_score = cov_score; out[b].lmid = lmid;
        // the set stands where the kernels appended it; what it replaced is garbage
        m->ls_live += n_local - m->ls_count_h[k];
        m->ls_start_h[k] = m->ls_pool_used; m->ls_count_h[k] = n_local;
        out[b].d_lmid = m->ls_pool + m->ls_pool_used; out[b].d_n_local = m->ls_count + k;
        m->ls_pool_used += n_local;
    }
    return OV2_OK;
}

// ---- pose-graph update of B maps: four launches whatever B, no synchronisation unless the headers are asked for -------
namespace {

// the update stage over a filled job table: the clear, the anchor scan, the landmarks, the poses
void pg_update_launches(ov2_ctx *c, const job_table &JT, int nmax, int lmax, int kmax, unsigned zmax)
{
    hipStream_t st = c->stream;
    const int B = JT.B;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gL((lmax + 255) / 256, B), gK((kmax + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mp_anchor_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mp_landmarks_kernel, gL, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mp_poses_kernel, gK, b256, 0, st, JT.dev);
}

void pg_update_record(ov2_map_pg_update &u, const int *H)
{
    u.n_kf_chain = H[PH_KF_CHAIN]; u.n_kf_younger = H[PH_KF_YOUNGER]; u.n_lm_moved = H[PH_LM_MOVED];
    memcpy(u.T_corr, (const double *)(H + MH_N) + 7, 7 * sizeof(double));
}

// both forms of the update call: dev = chain_Twc is a device array (and d_skip, if given, one byte per map in device memory)
ov2_status pg_update_impl(ov2_ctx *c, const char *who, bool dev, int B, ov2_map *const *maps, const int32_t *newkf,
                          const int32_t *chain_off, const int32_t *chain_kfid, const double *chain_Twc, const uint8_t *d_skip,
                          ov2_map_pg_update *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !newkf || !chain_off) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
    ov2_status s;
    int n_active = 0;
    if (chain_off[0] != 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: chain_off[0] must be 0", who);
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        const int n = chain_off[b + 1] - chain_off[b];
        if (n < 0) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: chain_off descends", b);
        if (!n) continue;
        if (!chain_kfid || !chain_Twc) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
        if ((s = batch_kf_alive(c, m, newkf[b], b)) != OV2_OK) return s;
        const int32_t *ids = chain_kfid + chain_off[b];
        for (int i = 0; i < n; ++i) {
            if ((s = batch_kf_alive(c, m, ids[i], b)) != OV2_OK) return s;
            if (i && ids[i] <= ids[i - 1]) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the listed keyframes do not ascend (%d after %d)", b, ids[i], ids[i - 1]);
        }
        if (ids[n - 1] != newkf[b])
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: the list ends in keyframe %d, not in the new keyframe %d", b, ids[n - 1], newkf[b]);
        ++n_active;
    }
    if (out) memset(out, 0, (size_t)B * sizeof(*out));
    if (!n_active) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t total = (size_t)chain_off[B];
    const size_t ids_bytes = (total * sizeof(int32_t) + 15) & ~(size_t)15;
    job_table JT;
    if ((s = JT.begin(c, B, 28, ids_bytes + (dev ? 0 : total * 7 * sizeof(double)))) != OV2_OK) return s;   // 28 ints = 14 doubles per map
    memcpy(JT.tail_host, chain_kfid, total * sizeof(int32_t));
    const double *d_Twc = chain_Twc;
    if (!dev) {
        memcpy(JT.tail_host + ids_bytes, chain_Twc, total * 7 * sizeof(double));
        d_Twc = (const double *)(JT.tail_dev + ids_bytes);
    }
    int nmax = 0, lmax = 0, kmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        map_job j = job_of(m, newkf[b], -1);
        j.pg_n = chain_off[b + 1] - chain_off[b];
        stage_block(j, m->tt_zero, j.pg_n ? m->tt_zero_bytes : 0);
        j.tt_old = m->tt_old;
        j.pg_kfid = (const int *)JT.tail_dev + chain_off[b];
        j.pg_Twc = d_Twc + 7 * (size_t)chain_off[b];
        j.pg_skip = d_skip ? d_skip + b : nullptr;
        JT.set(b, j);
        JT.host[b].pg_tmp = (double *)(JT.host[b].hdr_out + MH_N);
        if (!j.pg_n) continue;
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); kmax = std::max(kmax, m->max_kf); zmax = std::max(zmax, j.zero_vec16);
        m->last_valid = 0;   // its tables change under the last set-up: no update stage from it any more
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    pg_update_launches(c, JT, nmax, lmax, kmax, zmax);
    if (!out) return OV2_OK;   // fully asynchronous
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b)
        if (chain_off[b + 1] != chain_off[b]) pg_update_record(out[b], JT.hdr_host + (size_t)b * JT.stride);
    return OV2_OK;
}

// what the host knows of map b's chain without asking the device (Optimizer::assembleLocalPoseGraph :2368-2425 on the host
// copy of the keyframe states): ids = the loop keyframe after the walk-up, then the live keyframes up to newkf; empty = no chain
void lpg_chain(const ov2_map *m, int newkf, int kfloop_id, std::vector<int32_t> &ids)
{
    ids.clear();
    auto alive = [&](int k) { return k >= 0 && k < m->max_kf && m->kf_alive_h[k]; };
    if (!alive(newkf)) return;                              // a dead new keyframe
    int loop = std::max(kfloop_id, 0);                      // the walk-up stops at the first live keyframe (:2368-2371) ...
    while (loop < newkf && !alive(loop)) ++loop;
    if (loop >= newkf) return;                              // ... and one at or past newkf leaves fewer than two poses
    ids.push_back(loop);
    for (int k = loop + 1; k <= newkf; ++k)
        if (alive(k)) ids.push_back(k);
}

// [ids of every chain | newTwc of every map] behind the gathered headers; per map 28 ints of pg_tmp and the verdict (+ pad)
enum { LPG_EXTRA_INTS = 30, LPG_VERDICT = MH_N + 28 };

struct lpg_plan {
    std::vector<std::vector<int32_t>> ids;   // per map, empty = NO_CHAIN
    std::vector<size_t> off;                 // first pose of map b in the flat block (B + 1)
    int n_active = 0;
    size_t total() const { return off.back(); }
};

ov2_status lpg_validate(ov2_ctx *c, const char *who, int B, ov2_map *const *maps, const int32_t *newkf, const int32_t *kfloop_id,
                        const double *newTwc, lpg_plan &pl)
{
    if (B < 0 || !maps || !newkf || !kfloop_id || !newTwc) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument or B < 0", who);
    ov2_status s;
    pl.ids.resize((size_t)B);
    pl.off.assign((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        if ((s = batch_map_ok(c, maps[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        lpg_chain(maps[b], newkf[b], kfloop_id[b], pl.ids[b]);
        pl.off[b + 1] = pl.off[b] + pl.ids[b].size();
        pl.n_active += pl.ids[b].empty() ? 0 : 1;
    }
    return OV2_OK;
}

// the job table of the statement, its problem block in the ctx's own device block, and the assembly launch.
// Layout of the block: poses (7 x total) | T_ij (7 x total) | result records (one per map) | skip bytes (one per map)
struct lpg_block { double *pose, *Tij; ov2_pg_result *res; unsigned char *skip; };

ov2_status lpg_assemble(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, const double *newTwc, int stereo,
                        int32_t *d_n_pairs, const lpg_plan &pl, size_t host_tail, job_table &JT, lpg_block &K)
{
    ov2_status s;
    const size_t total = pl.total();
    const size_t o_T = (total * 7 * sizeof(double) + 255) & ~(size_t)255, o_res = 2 * o_T;
    const size_t o_skip = o_res + (((size_t)B * sizeof(ov2_pg_result) + 255) & ~(size_t)255);
    if ((s = ov2_dev_block(c, &c->lpg_dev, &c->lpg_dev_cap, o_skip + (size_t)B)) != OV2_OK) return s;
    unsigned char *blk = (unsigned char *)c->lpg_dev;
    K.pose = (double *)blk; K.Tij = (double *)(blk + o_T); K.res = (ov2_pg_result *)(blk + o_res); K.skip = blk + o_skip;
    const size_t ids_bytes = (total * sizeof(int32_t) + 15) & ~(size_t)15, up_bytes = ids_bytes + (size_t)B * 7 * sizeof(double);
    if ((s = JT.begin(c, B, LPG_EXTRA_INTS, up_bytes + host_tail)) != OV2_OK) return s;
    JT.tail_bytes = up_bytes;   // what goes up; the rest of the tail is the pinned landing area of the call's downloads
    memcpy(JT.tail_host + ids_bytes, newTwc, (size_t)B * 7 * sizeof(double));
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        const std::vector<int32_t> &ids = pl.ids[b];
        const int n = (int)ids.size();
        map_job j = job_of(m, newkf[b], -1);
        stage_block(j, m->tt_zero, n ? m->tt_zero_bytes : 0);
        j.tt_old = m->tt_old;
        j.lp_n = n; j.lp_stereo = stereo;
        j.lp_kfid = (const int *)JT.tail_dev + pl.off[b];
        j.lp_newTwc = (const double *)(JT.tail_dev + ids_bytes) + 7 * (size_t)b;
        j.lp_pose = K.pose + 7 * pl.off[b]; j.lp_Tij = K.Tij + 7 * pl.off[b];
        j.lp_skip = K.skip + b;
        j.lp_npairs = d_n_pairs ? d_n_pairs + b : nullptr;
        // the update stage reads the same block past the constant loop keyframe
        j.pg_n = n ? n - 1 : 0; j.pg_kfid = j.lp_kfid + 1; j.pg_Twc = j.lp_pose + 7; j.pg_skip = j.lp_skip;
        JT.set(b, j);
        JT.host[b].pg_tmp = (double *)(JT.host[b].hdr_out + MH_N);
        JT.host[b].lp_verdict = JT.host[b].hdr_out + LPG_VERDICT;
        if (n) memcpy((int32_t *)JT.tail_host + pl.off[b], ids.data(), (size_t)n * sizeof(int32_t));
        nmax = std::max(nmax, n);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mp_assemble_kernel, dim3((std::max(nmax, 1) + 255) / 256, B), dim3(256), 0, c->stream, JT.dev);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_map_pose_graph_update_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                      const int32_t *chain_off, const int32_t *chain_kfid, const double *chain_Twc,
                                                      ov2_map_pg_update *out)
{
    return pg_update_impl(c, "ov2_map_pose_graph_update_batch", false, B, maps, newkf, chain_off, chain_kfid, chain_Twc, nullptr, out);
}

extern "C" ov2_status ov2_map_pose_graph_update_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                          const int32_t *chain_off, const int32_t *chain_kfid, const double *d_chain_Twc,
                                                          const uint8_t *d_skip, ov2_map_pg_update *out)
{
    return pg_update_impl(c, "ov2_map_pose_graph_update_batch_dev", true, B, maps, newkf, chain_off, chain_kfid, d_chain_Twc, d_skip, out);
}

extern "C" ov2_status ov2_map_local_pose_graph_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                     const int32_t *kfloop_id, const double *newTwc, int stereo, const ov2_ba_options *o,
                                                     int32_t *d_n_pairs, ov2_map_local_pg *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    const char *who = "ov2_map_local_pose_graph_batch";
    ov2_status s;
    lpg_plan pl;
    if ((s = lpg_validate(c, who, B, maps, newkf, kfloop_id, newTwc, pl)) != OV2_OK) return s;
    if (B > OV2_PG_MAX_BATCH) return ov2_set_err(c, OV2_ERR_INVALID, "%s: B %d above %d", who, B, OV2_PG_MAX_BATCH);
    ov2_ba_options od;
    if (!o) {   // Optimizer::localPoseGraphOptions (:2442-2446)
        ov2_ba_default_options(&od, 5.9915f);
        od.max_iters = 10; od.function_tolerance = 1e-4;
        o = &od;
    }
    if (o->max_iters < 0 || o->max_iters > OV2_BA_MAX_LOG - 1)
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: max_iters %d outside [0, %d]", who, o->max_iters, OV2_BA_MAX_LOG - 1);
    if (out) {
        memset(out, 0, (size_t)B * sizeof(*out));
        for (int b = 0; b < B; ++b) {
            out[b].verdict = OV2_LPG_NO_CHAIN; out[b].kfloop_id = -1;
            out[b].result.termination = OV2_BA_TERM_SKIPPED;
        }
    }
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (!pl.n_active) {   // no work on the device beyond the refused counts
        if (d_n_pairs) OV2_HIP(c, hipMemsetAsync(d_n_pairs, 0, (size_t)B * sizeof(int32_t), st));
        return OV2_OK;
    }
    job_table JT;
    lpg_block K;
    if ((s = lpg_assemble(c, B, maps, newkf, newTwc, stereo ? 1 : 0, d_n_pairs, pl, out ? (size_t)B * sizeof(ov2_pg_result) : 0, JT, K)) != OV2_OK)
        return s;
    // the solve: one graph per map that has a chain, in batch order; structure from the host, values where the assembly left them
    std::vector<ov2_pg_problem> P;
    std::vector<int> act;
    const size_t total = pl.total();
    std::vector<int32_t> ei(total), ej(total);
    std::vector<uint8_t> cst(total, 0);
    int nmax = 0, lmax = 0, kmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        const int n = (int)pl.ids[b].size();
        if (!n) continue;
        const size_t o0 = pl.off[b];
        for (int i = 0; i + 1 < n; ++i) { ei[o0 + i] = i; ej[o0 + i] = i + 1; }
        ei[o0 + n - 1] = 0; ej[o0 + n - 1] = n - 1;
        cst[o0] = 1;
        ov2_pg_problem G;
        G.n_pose = n; G.pose = K.pose + 7 * o0; G.pose_const = cst.data() + o0;
        G.n_edge = n; G.edge_i = ei.data() + o0; G.edge_j = ej.data() + o0; G.T_ij = K.Tij + 7 * o0;
        P.push_back(G); act.push_back(b);
        ov2_map *m = maps[b];
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); kmax = std::max(kmax, m->max_kf);
        zmax = std::max(zmax, JT.host[b].zero_vec16);
        m->last_valid = 0;   // its tables change under the last set-up: no update stage from it any more
    }
    if ((s = ov2_pg_solve_dev(c, who, (int)P.size(), P.data(), o, K.res)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mp_gate_kernel, dim3((B + 63) / 64), dim3(64), 0, st, JT.dev, B);
    pg_update_launches(c, JT, nmax, lmax, kmax, zmax);
    OV2_HIP(c, hipGetLastError());
    if (!out) return OV2_OK;   // fully asynchronous
    OV2_LAUNCH(c, OV2_K_MAP, mb_hdr_gather_kernel, dim3(1, B), dim3(64), 0, st, JT.dev);
    unsigned char *res_host = JT.tail_host + ((JT.tail_bytes + 255) & ~(size_t)255);
    OV2_HIP(c, hipMemcpyAsync(res_host, K.res, P.size() * sizeof(ov2_pg_result), hipMemcpyDeviceToHost, st));
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (size_t a = 0; a < act.size(); ++a) {
        const int b = act[a];
        const int *H = JT.hdr_host + (size_t)b * JT.stride;
        ov2_map_local_pg &r = out[b];
        r.verdict = H[LPG_VERDICT]; r.kfloop_id = pl.ids[b][0]; r.n_pose = (int)pl.ids[b].size();
        if (r.verdict == OV2_LPG_DONE) pg_update_record(r.update, H);
        memcpy(&r.result, res_host + a * sizeof(ov2_pg_result), sizeof(ov2_pg_result));
    }
    return OV2_OK;
}

// test hook: the assembly stage of ov2_map_local_pose_graph_batch alone, downloaded.  chain_off (B + 1) receives where map
// b's poses and edges start, kfid / pose / T_ij (cap poses) the chains; a map without a chain lists nothing.
extern "C" ov2_status ov2_map_local_pose_graph_assemble(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf,
                                                        const int32_t *kfloop_id, const double *newTwc, int cap, int32_t *chain_off,
                                                        int32_t *kfid, double *pose, double *T_ij)
{
    if (!c) return OV2_ERR_INVALID;
    const char *who = "ov2_map_local_pose_graph_assemble";
    if (B <= 0 || !chain_off || !kfid || !pose || !T_ij) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument or B <= 0", who);
    ov2_status s;
    lpg_plan pl;
    if ((s = lpg_validate(c, who, B, maps, newkf, kfloop_id, newTwc, pl)) != OV2_OK) return s;
    const size_t total = pl.total();
    if (total > (size_t)std::max(cap, 0)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: %zu poses, room for %d", who, total, cap);
    for (int b = 0; b <= B; ++b) chain_off[b] = (int32_t)pl.off[b];
    for (int b = 0; b < B; ++b) std::copy(pl.ids[b].begin(), pl.ids[b].end(), kfid + pl.off[b]);
    if (!total) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    job_table JT;
    lpg_block K;
    if ((s = lpg_assemble(c, B, maps, newkf, newTwc, 0, nullptr, pl, 2 * total * 7 * sizeof(double), JT, K)) != OV2_OK) return s;
    hipStream_t st = c->stream;
    unsigned char *land = JT.tail_host + ((JT.tail_bytes + 255) & ~(size_t)255);
    OV2_HIP(c, hipMemcpyAsync(land, K.pose, total * 7 * sizeof(double), hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipMemcpyAsync(land + total * 7 * sizeof(double), K.Tij, total * 7 * sizeof(double), hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(pose, land, total * 7 * sizeof(double));
    memcpy(T_ij, land + total * 7 * sizeof(double), total * 7 * sizeof(double));
    return OV2_OK;
}

// ---- map-point merges of B maps: eight launches whatever B and the pair counts are (clear, mark, count, three of the scan,
// index, walk), no synchronisation unless headers or host-side statuses are asked for ---------------------------------------
namespace {

ov2_status merge_batch_impl(ov2_ctx *c, const char *who, bool dev, int B, ov2_map *const *maps, const int32_t *pair_off,
                            const int32_t *prev, const int32_t *nw, const uint8_t *cur, const int32_t *d_n_pairs, ov2_map_merge *out,
                            uint8_t *status)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !pair_off) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
    if (pair_off[0] != 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: pair_off[0] must be 0", who);
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        if (pair_off[b + 1] < pair_off[b]) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: pair_off descends", b);
        if (m->snap_kf_pose)   // the snapshot does not cover obs_lm: a restore could not undo a relabel
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d holds a saved state: its rows cannot be relabelled", b);
    }
    const size_t total = (size_t)pair_off[B];
    if (total && (!prev || !nw)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null pair list", who);
    if (out) memset(out, 0, (size_t)B * sizeof(*out));
    if (!total) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // host form: [statuses | prev | new | cur_obs] behind the gathered headers, so that headers and statuses come back in one copy
    const size_t st_bytes = (total + 15) & ~(size_t)15, id_bytes = (total * sizeof(int32_t) + 15) & ~(size_t)15;
    job_table JT;
    if ((s = JT.begin(c, B, 0, dev ? 0 : 2 * st_bytes + 2 * id_bytes)) != OV2_OK) return s;
    const int32_t *d_prev = prev, *d_new = nw;
    const uint8_t *d_cur = cur;
    uint8_t *d_status = status;
    if (!dev) {
        memcpy(JT.tail_host + st_bytes, prev, total * sizeof(int32_t));
        memcpy(JT.tail_host + st_bytes + id_bytes, nw, total * sizeof(int32_t));
        if (cur) memcpy(JT.tail_host + st_bytes + 2 * id_bytes, cur, total);
        d_status = status ? JT.tail_dev : nullptr;
        d_prev = (const int32_t *)(JT.tail_dev + st_bytes); d_new = (const int32_t *)(JT.tail_dev + st_bytes + id_bytes);
        d_cur = cur ? JT.tail_dev + st_bytes + 2 * id_bytes : nullptr;
    }
    int nmax = 0, lmax = 0, pmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        map_job j = job_of(m, -1, -1);
        j.mg_seg = pair_off[b + 1] - pair_off[b];
        stage_block(j, m->mg_zero, j.mg_seg ? m->mg_zero_bytes : 0);
        j.mg_prev = d_prev + pair_off[b]; j.mg_new = d_new + pair_off[b];
        j.mg_cur = d_cur ? d_cur + pair_off[b] : nullptr;
        j.mg_n_dev = d_n_pairs ? d_n_pairs + b : nullptr;
        j.mg_status = d_status ? d_status + pair_off[b] : nullptr;
        j.mg_cnt = m->mg_cnt; j.mg_fill = m->mg_fill; j.mg_next = m->mg_next; j.mg_stamp = m->mg_stamp; j.mg_mark = m->mg_mark;
        j.mg_start = m->mg_start; j.mg_rows = m->mg_rows;
        JT.set(b, j);
        if (!j.mg_seg) continue;   // an empty list leaves the map alone
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); pmax = std::max(pmax, j.mg_seg); zmax = std::max(zmax, j.zero_vec16);
        m->last_valid = 0;   // its tables change under the last set-up: no update stage from it any more
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gP((pmax + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_mark_kernel, gP, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_count_kernel, gN, b256, 0, st, JT.dev);
    if ((s = exclusive_scan<int>(c, JT, SC_MG, lmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mg_index_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_walk_kernel, dim3(1, B), dim3(MG_THREADS), 0, st, JT.dev);
    OV2_HIP(c, hipGetLastError());
    if (!out && (dev || !status)) return OV2_OK;   // asynchronous: nothing to hand to the host
    if (dev) {
        if ((s = JT.fetch_headers()) != OV2_OK) return s;
    } else {   // the headers and, right behind them, the statuses
        const size_t bytes = (size_t)(JT.tail_host - (unsigned char *)JT.hdr_host) + total;
        OV2_HIP(c, hipMemcpyAsync(JT.hdr_host, JT.hdr_dev, bytes, hipMemcpyDeviceToHost, st));
        OV2_HIP(c, hipStreamSynchronize(st));
        if (status) memcpy(status, JT.tail_host, total);
    }
    for (int b = 0; b < B && out; ++b) {
        const int *H = JT.hdr_host + (size_t)b * JT.stride;
        out[b].n_pairs = H[GH_PAIRS]; out[b].n_merged = H[GH_MERGED]; out[b].n_skipped = H[GH_SKIPPED];
        out[b].n_rows_moved = H[GH_MOVED]; out[b].n_rows_conflict = H[GH_CONFLICT];
    }
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_map_merge_points_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *pair_off, const int32_t *prev_lmid,
                                                 const int32_t *new_lmid, const uint8_t *cur_obs, ov2_map_merge *out, uint8_t *pair_status)
{
    return merge_batch_impl(c, "ov2_map_merge_points_batch", false, B, maps, pair_off, prev_lmid, new_lmid, cur_obs, nullptr, out, pair_status);
}

extern "C" ov2_status ov2_map_merge_points_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *pair_off,
                                                     const int32_t *d_prev_lmid, const int32_t *d_new_lmid, const uint8_t *d_cur_obs,
                                                     const int32_t *d_n_pairs, ov2_map_merge *out, uint8_t *d_pair_status)
{
    return merge_batch_impl(c, "ov2_map_merge_points_batch_dev", true, B, maps, pair_off, d_prev_lmid, d_new_lmid, d_cur_obs, d_n_pairs, out,
                            d_pair_status);
}

// ---- structure-only BA of B maps: eight launches whatever B and the list lengths are (clear, mark, count, three of the scan,
// index, solve), no synchronisation unless the records are asked for ---------------------------------------------------------
namespace {

ov2_status grow_sba(ov2_map *m, int entries)
{
    ov2_ctx *c = m->c;
    if (entries <= m->sb_cap) return OV2_OK;
    OV2_HIP(c, hipStreamSynchronize(c->stream));   // an earlier call may still be working in the old block
    if (m->sb_ws) OV2_HIP(c, hipFree(m->sb_ws));
    m->sb_ws = nullptr; m->sb_cap = 0;
    const int want = entries + entries / 2 + 64;
    if (hipMalloc((void **)&m->sb_ws, (size_t)want * (SP_N * sizeof(double) + sizeof(int))) != hipSuccess)
        return ov2_set_err(c, OV2_ERR_NOMEM, "structure-only BA block of %d entries", want);
    m->sb_cap = want;
    return OV2_OK;
}

ov2_status structure_ba_impl(ov2_ctx *c, const char *who, bool dev, int B, ov2_map *const *maps, const int32_t *lm_off, const int32_t *lmid,
                             const int32_t *d_n, const uint8_t *d_status, const ov2_map_sba_cam *cam, const ov2_ba_options *o,
                             ov2_map_sba *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps || !lm_off) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
    if (lm_off[0] != 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: lm_off[0] must be 0", who);
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        if ((s = batch_map_ok(c, maps[b], b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, maps, b)) != OV2_OK) return s;
        if (lm_off[b + 1] < lm_off[b]) return ov2_set_err(c, OV2_ERR_INVALID, "map %d: lm_off descends", b);
    }
    if (o && (o->max_iters < 0 || o->max_iters > OV2_BA_MAX_LOG - 1))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: max_iters %d outside [0, %d]", who, o->max_iters, OV2_BA_MAX_LOG - 1);
    const size_t total = (size_t)lm_off[B];
    if (total && (!lmid || !cam || !o)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null id list, cameras or options", who);
    if (out) {
        memset(out, 0, (size_t)B * sizeof(*out));
        for (int b = 0; b < B; ++b) out[b].termination = OV2_BA_TERM_SKIPPED;
    }
    if (!total) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    for (int b = 0; b < B; ++b)
        if (lm_off[b + 1] > lm_off[b] && (s = grow_sba(maps[b], lm_off[b + 1] - lm_off[b])) != OV2_OK) return s;
    // behind the gathered records: [cameras | ids (host form)]
    static_assert(sizeof(ov2_map_sba) % 8 == 0 && sizeof(ov2_map_sba) >= MH_N * sizeof(int), "the record stands where a header stands");
    const size_t cam_bytes = ((size_t)B * sizeof(ov2_map_sba_cam) + 15) & ~(size_t)15;
    job_table JT;
    if ((s = JT.begin(c, B, (int)(sizeof(ov2_map_sba) / sizeof(int)) - MH_N, cam_bytes + (dev ? 0 : total * sizeof(int32_t)))) != OV2_OK) return s;
    memcpy(JT.tail_host, cam, (size_t)B * sizeof(ov2_map_sba_cam));
    const int32_t *d_ids = lmid;
    if (!dev) {
        memcpy(JT.tail_host + cam_bytes, lmid, total * sizeof(int32_t));
        d_ids = (const int32_t *)(JT.tail_dev + cam_bytes);
    }
    int nmax = 0, lmax = 0, pmax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        map_job j = job_of(m, -1, -1);
        j.mg_seg = lm_off[b + 1] - lm_off[b];
        stage_block(j, m->mg_zero, j.mg_seg ? m->mg_zero_bytes : 0);
        j.sb_on = 1;
        j.mg_new = d_ids + lm_off[b];
        j.mg_n_dev = d_n ? d_n + b : nullptr;
        j.sb_status = d_status ? d_status + lm_off[b] : nullptr;
        j.sb_cam = (const double *)(JT.tail_dev + (size_t)b * sizeof(ov2_map_sba_cam));
        j.sb_pt = (double *)m->sb_ws;
        j.sb_lm = (int *)(m->sb_ws + (size_t)m->sb_cap * SP_N * sizeof(double));
        j.mg_cnt = m->mg_cnt; j.mg_fill = m->mg_fill; j.mg_next = m->mg_next; j.mg_stamp = m->mg_stamp; j.mg_mark = m->mg_mark;
        j.mg_start = m->mg_start; j.mg_rows = m->mg_rows;
        JT.set(b, j);
        if (!j.mg_seg) continue;   // an empty list leaves the map alone
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); pmax = std::max(pmax, j.mg_seg); zmax = std::max(zmax, j.zero_vec16);
        m->last_valid = 0;   // the sorted rows go where its set-up left its offsets: no update stage from it any more
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    sb_opt so;
    so.huber_a = o->huber_delta; so.ftol = o->function_tolerance; so.initial_radius = o->initial_radius; so.max_radius = o->max_radius;
    so.min_radius = o->min_radius; so.min_d = o->min_lm_diagonal; so.max_d = o->max_lm_diagonal; so.min_rel = o->min_relative_decrease;
    so.ptol = o->parameter_tolerance; so.gtol = o->gradient_tolerance; so.max_iters = o->max_iters; so.jacobi = o->jacobi_scaling;
    so.max_invalid = o->max_consecutive_invalid_steps;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gP((pmax + 255) / 256, B), b256(256);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::min(64u, (zmax + 255) / 256), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_mark_kernel, gP, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_count_kernel, gN, b256, 0, st, JT.dev);
    if ((s = exclusive_scan<int>(c, JT, SC_MG, lmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mg_index_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP_SBA, sb_solve_kernel, dim3(1, B), dim3(SB_THREADS), 0, st, JT.dev, so);
    OV2_HIP(c, hipGetLastError());
    if (!out) return OV2_OK;   // asynchronous: nothing to hand to the host
    if ((s = JT.fetch_headers()) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) memcpy(&out[b], JT.hdr_host + (size_t)b * JT.stride, sizeof(ov2_map_sba));
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_map_structure_ba_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *lm_off, const int32_t *lmid,
                                                 const ov2_map_sba_cam *cam, const ov2_ba_options *o, ov2_map_sba *out)
{
    return structure_ba_impl(c, "ov2_map_structure_ba_batch", false, B, maps, lm_off, lmid, nullptr, nullptr, cam, o, out);
}

extern "C" ov2_status ov2_map_structure_ba_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *lm_off, const int32_t *d_lmid,
                                                     const int32_t *d_n, const uint8_t *d_status, const ov2_map_sba_cam *cam,
                                                     const ov2_ba_options *o, ov2_map_sba *out)
{
    return structure_ba_impl(c, "ov2_map_structure_ba_batch_dev", true, B, maps, lm_off, d_lmid, d_n, d_status, cam, o, out);
}

// ---- local-map matching from the mirrors: gather (twelve launches whatever B and the list lengths are: clear, mark, count,
// three of the per-map scan, index, entry counts + poses, three of the flat scan, fill), then the matcher's own path --------
namespace {

struct gather_args {
    int B; ov2_map *const *maps; const int32_t *newkf, *nb3dkps, *kp_off, *kp_lmid, *grid_ptr, *grid_kp, *cand_off, *cand_lmid;
    const double *K; int img_w, img_h, cell; const ov2_cam_model *cam;
};

// what a call leaves in the ctx scratch behind the gathered arrays: the matcher's work array and the results
struct gather_extra { uint64_t *work; int32_t *match_cand; float *match_dist; int32_t *prev_lmid, *new_lmid, *n_pairs; };

// nothing_to_do: B == 0 or no keypoint at all (OV2_OK, nothing enqueued, *in describes the empty call)
ov2_status gather_impl(ov2_ctx *c, const char *who, const gather_args &A, ov2_match_batch_input *in, const int32_t **d_kp_lmid,
                       const int32_t **d_cand_lmid, gather_extra *X, size_t result_host_bytes, unsigned char **result_host,
                       bool *nothing_to_do)
{
    *nothing_to_do = true;
    if (!c) return OV2_ERR_INVALID;
    if (!in) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null output", who);
    memset(in, 0, sizeof(*in));
    const int B = A.B;
    if (B == 0) return OV2_OK;
    if (B < 0 || !A.maps || !A.newkf || !A.nb3dkps || !A.kp_off || !A.cand_off || !A.K)
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
    if (A.kp_off[0] != 0 || A.cand_off[0] != 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: offsets must start at 0", who);
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        const ov2_map *m = A.maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if ((s = batch_map_once(c, A.maps, b)) != OV2_OK) return s;
        if (!m->obs_hasdesc) return ov2_set_err(c, OV2_ERR_INVALID, "%s: map %d has no match columns", who, b);
        if ((s = batch_kf_alive(c, m, A.newkf[b], b)) != OV2_OK) return s;
        if (A.kp_off[b + 1] < A.kp_off[b] || A.cand_off[b + 1] < A.cand_off[b])
            return ov2_set_err(c, OV2_ERR_INVALID, "%s: frame %d has a negative count", who, b);
    }
    const int nkp = A.kp_off[B], nc = A.cand_off[B];
    if ((nkp && !A.kp_lmid) || (nc && !A.cand_lmid)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null id list", who);
    if (A.cell <= 0 || A.img_w <= 0 || A.img_h <= 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: bad image / cell size", who);
    const int nbw = (int)ceilf((float)A.img_w / (float)A.cell), nbh = (int)ceilf((float)A.img_h / (float)A.cell);
    const size_t ncells = (size_t)nbw * nbh, ng_ptr = (size_t)B * ncells + 1;
    size_t n_g = 0;
    if (nkp && nc) {   // the grid is read by the matcher only
        if (!A.grid_ptr) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null grid", who);
        if (A.grid_ptr[0] != 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: grid_ptr must start at 0", who);
        for (size_t i = 0; i + 1 < ng_ptr; ++i)
            if (A.grid_ptr[i + 1] < A.grid_ptr[i]) return ov2_set_err(c, OV2_ERR_INVALID, "%s: grid_ptr decreases", who);
        n_g = (size_t)A.grid_ptr[ng_ptr - 1];
        if (n_g && !A.grid_kp) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null grid", who);
        for (int b = 0; b < B; ++b) {
            const int nb = A.kp_off[b + 1] - A.kp_off[b];
            for (int g = A.grid_ptr[(size_t)b * ncells]; g < A.grid_ptr[(size_t)(b + 1) * ncells]; ++g)
                if (A.grid_kp[g] < 0 || A.grid_kp[g] >= nb)
                    return ov2_set_err(c, OV2_ERR_INVALID, "%s: grid entry %d of frame %d outside its %d keypoints", who, A.grid_kp[g], b, nb);
        }
    }
    // a landmark at most once per list (the reference's lists are keyed by lmid): that bounds the gathered rows by the tables'
    for (int b = 0; b < B; ++b) {
        ov2_map *m = A.maps[b];
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t *ids = pass ? A.cand_lmid : A.kp_lmid;
            const int i0 = pass ? A.cand_off[b] : A.kp_off[b], i1 = pass ? A.cand_off[b + 1] : A.kp_off[b + 1];
            if (m->gt_gen == 0x7fffffff) { memset(m->gt_seen_h, 0, (size_t)m->max_lm * sizeof(int)); m->gt_gen = 0; }
            const int gen = ++m->gt_gen;
            for (int i = i0; i < i1; ++i) {
                const int l = ids[i];
                if (l < 0 || l >= m->max_lm) continue;
                if (m->gt_seen_h[l] == gen)
                    return ov2_set_err(c, OV2_ERR_INVALID, "%s: landmark %d twice among the %s of frame %d", who, l, pass ? "candidates" : "keypoints", b);
                m->gt_seen_h[l] = gen;
            }
        }
    }
    in->B = B; in->n_kp = nkp; in->n_cand = nc; in->img_w = A.img_w; in->img_h = A.img_h; in->cell = A.cell; in->cam = A.cam;
    for (int i = 0; i < 4; ++i) in->K[i] = A.K[i];
    if (nkp == 0) return OV2_OK;
    *nothing_to_do = false;
    OV2_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    // the id lists behind the job records: one pinned image, one upload
    enum { T_NB3D = 0, T_KPOFF, T_CANDOFF, T_KFOFF, T_KPLM, T_CANDLM, T_GPTR, T_GKP, T_N };
    const size_t t_bytes[T_N] = {(size_t)B * 4, ((size_t)B + 1) * 4, ((size_t)B + 1) * 4, ((size_t)B + 1) * 4, (size_t)nkp * 4, (size_t)nc * 4,
                                 (nkp && nc) ? ng_ptr * 4 : 0, n_g * 4};
    size_t t_off[T_N], tail = 0;
    for (int i = 0; i < T_N; ++i) { t_off[i] = tail; tail += pad(t_bytes[i]); }
    job_table JT;
    if ((s = JT.begin(c, B + 4, 0, tail + pad(result_host_bytes))) != OV2_OK) return s;
    JT.tail_bytes = tail;   // what goes up; the rest of the block takes the results on their way back
    if (result_host) *result_host = JT.tail_host + tail;
    // the gathered arrays, sized from what the host knows: an entry lists at most the live rows of its landmark
    size_t rows = 0, kfs = 0;
    for (int b = 0; b < B; ++b) { rows += (size_t)A.maps[b]->n_obs; kfs += (size_t)A.maps[b]->max_kf; }
    if (rows > 0x7fffffff / 2 || kfs > 0x7fffffff / 8) return ov2_set_err(c, OV2_ERR_INVALID, "%s: the batch holds too many rows", who);
    enum { G_TWC = 0, G_KPPX, G_KPDPTR, G_KPKPTR, G_KPKF, G_KPKFPX, G_KPDESC, G_CWPT, G_CDPTR, G_CKPTR, G_CKF, G_CDESC, G_KFTWC,
           G_BLK0, G_BLK1, G_BLK2, G_BLK3, G_WORK, G_MC, G_MD, G_PREV, G_NEW, G_NP, G_N };
    const size_t blk_kp = ((size_t)nkp + 1023) / 1024 + 1, blk_c = ((size_t)nc + 1023) / 1024 + 1;
    const size_t g_bytes[G_N] = {(size_t)B * 56, (size_t)nkp * 8, ((size_t)nkp + 1) * 4, ((size_t)nkp + 1) * 4, rows * 4, rows * 8, rows * 32,
                                 (size_t)nc * 24, ((size_t)nc + 1) * 4, ((size_t)nc + 1) * 4, rows * 4, rows * 32, kfs * 56,
                                 blk_kp * 4, blk_kp * 4, blk_c * 4, blk_c * 4,
                                 X ? (size_t)nkp * 8 : 0, X ? (size_t)nkp * 4 : 0, X ? (size_t)nkp * 4 : 0, X ? (size_t)nkp * 4 : 0,
                                 X ? (size_t)nkp * 4 : 0, X ? (size_t)B * 4 : 0};
    size_t g_off[G_N], total = pad(JT.tail_off + tail);
    for (int i = 0; i < G_N; ++i) { g_off[i] = total; total += pad(g_bytes[i]); }
    void *scr = nullptr;
    if ((s = ov2_scratch(c, total, &scr)) != OV2_OK) return s;
    unsigned char *D = (unsigned char *)scr;
    // the job records and the id lists go to the scratch block, not to the staging block's device twin: what the call hands
    // out must outlive the next call that stages
    JT.hdr_dev = (int *)(D + ((unsigned char *)JT.hdr_host - (unsigned char *)JT.host));
    JT.dev = (const map_job *)D; JT.tail_dev = D + JT.tail_off;
    auto tail_put = [&](int k, const void *src) { if (t_bytes[k] && src) memcpy(JT.tail_host + t_off[k], src, t_bytes[k]); };
    tail_put(T_NB3D, A.nb3dkps); tail_put(T_KPOFF, A.kp_off); tail_put(T_CANDOFF, A.cand_off); tail_put(T_KPLM, A.kp_lmid);
    tail_put(T_CANDLM, A.cand_lmid); tail_put(T_GPTR, A.grid_ptr); tail_put(T_GKP, A.grid_kp);
    int32_t *kf_off_h = (int32_t *)(JT.tail_host + t_off[T_KFOFF]);
    kf_off_h[0] = 0;
    for (int b = 0; b < B; ++b) kf_off_h[b + 1] = kf_off_h[b] + A.maps[b]->max_kf;
    gather_out G;
    G.Twc = (double *)(D + g_off[G_TWC]); G.kp_px = (float2 *)(D + g_off[G_KPPX]); G.kp_desc_ptr = (int *)(D + g_off[G_KPDPTR]);
    G.kp_kf_ptr = (int *)(D + g_off[G_KPKPTR]); G.kp_kfids = (int *)(D + g_off[G_KPKF]); G.kp_kf_px = (float2 *)(D + g_off[G_KPKFPX]);
    G.kp_descs = (uint4 *)(D + g_off[G_KPDESC]); G.cand_wpt = (double *)(D + g_off[G_CWPT]); G.cand_desc_ptr = (int *)(D + g_off[G_CDPTR]);
    G.cand_kf_ptr = (int *)(D + g_off[G_CKPTR]); G.cand_kfids = (int *)(D + g_off[G_CKF]); G.cand_descs = (uint4 *)(D + g_off[G_CDESC]);
    G.kf_Twc = (double *)(D + g_off[G_KFTWC]); G.cap_rows = (int)rows;
    const int32_t *dkp = (const int32_t *)(JT.tail_dev + t_off[T_KPLM]), *dcand = (const int32_t *)(JT.tail_dev + t_off[T_CANDLM]);
    int nmax = 0, lmax = 0, emax = 0; unsigned zmax = 0;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = A.maps[b];
        map_job j = job_of(m, A.newkf[b], -1);
        j.gt_on = 1;
        j.gt_nkp = A.kp_off[b + 1] - A.kp_off[b]; j.gt_ncand = A.cand_off[b + 1] - A.cand_off[b];
        j.gt_kp0 = A.kp_off[b]; j.gt_cand0 = A.cand_off[b]; j.gt_kf0 = kf_off_h[b];
        j.gt_kp_lmid = dkp + A.kp_off[b]; j.gt_cand_lmid = dcand + A.cand_off[b];
        j.mg_seg = j.gt_nkp + j.gt_ncand;
        stage_block(j, m->mg_zero, j.mg_seg ? m->mg_zero_bytes : 0);
        j.mg_cnt = m->mg_cnt; j.mg_fill = m->mg_fill; j.mg_next = m->mg_next; j.mg_stamp = m->mg_stamp; j.mg_mark = m->mg_mark;
        j.mg_start = m->mg_start; j.mg_rows = m->mg_rows;
        JT.set(b, j);
        nmax = std::max(nmax, m->n_obs); lmax = std::max(lmax, m->max_lm); emax = std::max(emax, j.mg_seg); zmax = std::max(zmax, j.zero_vec16);
    }
    int *scan_arr[4] = {G.kp_kf_ptr, G.kp_desc_ptr, G.cand_kf_ptr, G.cand_desc_ptr};
    for (int q = 0; q < 4; ++q) {   // the flat scans: four records behind the maps'
        map_job j;
        memset(&j, 0, sizeof(j));
        j.gt_scan = scan_arr[q]; j.gt_scan_n = q < 2 ? nkp : nc;
        j.blk = D + g_off[G_BLK0 + q];
        JT.set(B + q, j);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    job_table MJ = JT, SJ = JT;
    MJ.B = B; SJ.B = 4; SJ.dev = JT.dev + B;
    const dim3 gN((std::max(nmax, 1) + 255) / 256, B), gE((std::max(emax, 1) + 255) / 256, B), b256(256);
    const dim3 gQ(((size_t)std::max(emax, 1) * GT_SUB + 255) / 256, B);
    OV2_LAUNCH(c, OV2_K_MAP, mb_zero_kernel, dim3(std::max(1u, std::min(64u, (zmax + 255) / 256)), B), b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_mark_kernel, gE, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, mg_count_kernel, gN, b256, 0, st, JT.dev);
    if ((s = exclusive_scan<int>(c, MJ, SC_MG, lmax)) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mg_index_kernel, gN, b256, 0, st, JT.dev);
    OV2_LAUNCH(c, OV2_K_MAP, gt_count_kernel, gQ, b256, 0, st, JT.dev, G);
    if ((s = exclusive_scan<int>(c, SJ, SC_GT, std::max(nkp, std::max(nc, 1)))) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, gt_fill_kernel, gQ, b256, 0, st, JT.dev, G);
    OV2_HIP(c, hipGetLastError());
    in->Twc = G.Twc; in->nb3dkps = (const int32_t *)(JT.tail_dev + t_off[T_NB3D]);
    in->kp_off = (const int32_t *)(JT.tail_dev + t_off[T_KPOFF]); in->cand_off = (const int32_t *)(JT.tail_dev + t_off[T_CANDOFF]);
    in->kf_off = (const int32_t *)(JT.tail_dev + t_off[T_KFOFF]);
    in->kp_px = (const float *)G.kp_px; in->kp_desc_ptr = G.kp_desc_ptr; in->kp_descs = (const uint8_t *)G.kp_descs;
    in->kp_kf_ptr = G.kp_kf_ptr; in->kp_kfids = G.kp_kfids; in->kp_kf_px = (const float *)G.kp_kf_px;
    in->grid_ptr = (const int32_t *)(JT.tail_dev + t_off[T_GPTR]); in->grid_kp = (const int32_t *)(JT.tail_dev + t_off[T_GKP]);
    in->cand_wpt = G.cand_wpt; in->cand_desc_ptr = G.cand_desc_ptr; in->cand_descs = (const uint8_t *)G.cand_descs;
    in->cand_kf_ptr = G.cand_kf_ptr; in->cand_kfids = G.cand_kfids; in->kf_Twc = G.kf_Twc;
    if (d_kp_lmid) *d_kp_lmid = dkp;
    if (d_cand_lmid) *d_cand_lmid = dcand;
    if (X) {
        X->work = (uint64_t *)(D + g_off[G_WORK]); X->match_cand = (int32_t *)(D + g_off[G_MC]); X->match_dist = (float *)(D + g_off[G_MD]);
        X->prev_lmid = (int32_t *)(D + g_off[G_PREV]); X->new_lmid = (int32_t *)(D + g_off[G_NEW]); X->n_pairs = (int32_t *)(D + g_off[G_NP]);
    }
    return OV2_OK;
}

gather_args gather_args_of(int B, ov2_map *const *maps, const int32_t *newkf, const int32_t *nb3dkps, const int32_t *kp_off,
                           const int32_t *kp_lmid, const int32_t *grid_ptr, const int32_t *grid_kp, const int32_t *cand_off,
                           const int32_t *cand_lmid, const double *K, int img_w, int img_h, int cell, const ov2_cam_model *cam)
{
    return gather_args{B, maps, newkf, nb3dkps, kp_off, kp_lmid, grid_ptr, grid_kp, cand_off, cand_lmid, K, img_w, img_h, cell, cam};
}

}  // namespace

extern "C" ov2_status ov2_map_match_gather_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, const int32_t *nb3dkps,
                                                     const int32_t *kp_off, const int32_t *kp_lmid, const int32_t *grid_ptr,
                                                     const int32_t *grid_kp, const int32_t *cand_off, const int32_t *cand_lmid,
                                                     const double *K, int img_w, int img_h, int cell, const ov2_cam_model *cam,
                                                     ov2_match_batch_input *out, const int32_t **d_kp_lmid, const int32_t **d_cand_lmid)
{
    bool nothing;
    if (d_kp_lmid) *d_kp_lmid = nullptr;
    if (d_cand_lmid) *d_cand_lmid = nullptr;
    return gather_impl(c, "ov2_map_match_gather_batch_dev",
                       gather_args_of(B, maps, newkf, nb3dkps, kp_off, kp_lmid, grid_ptr, grid_kp, cand_off, cand_lmid, K, img_w, img_h, cell, cam),
                       out, d_kp_lmid, d_cand_lmid, nullptr, 0, nullptr, &nothing);
}

extern "C" ov2_status ov2_map_match_local_batch_dev(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, const int32_t *nb3dkps,
                                                    const int32_t *kp_off, const int32_t *kp_lmid, const int32_t *grid_ptr,
                                                    const int32_t *grid_kp, const int32_t *cand_off, const int32_t *cand_lmid,
                                                    const double *K, int img_w, int img_h, int cell, const ov2_cam_model *cam,
                                                    float fmaxprojerr, float fdistratio, int pairs, ov2_map_match_local *out)
{
    if (!c) return OV2_ERR_INVALID;
    if (!out) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_match_local_batch_dev: null output");
    memset(out, 0, sizeof(*out));
    ov2_match_batch_input in;
    gather_extra X;
    const int32_t *dkp = nullptr, *dcand = nullptr;
    bool nothing;
    ov2_status s = gather_impl(c, "ov2_map_match_local_batch_dev",
                               gather_args_of(B, maps, newkf, nb3dkps, kp_off, kp_lmid, grid_ptr, grid_kp, cand_off, cand_lmid, K, img_w, img_h, cell, cam),
                               &in, &dkp, &dcand, &X, 0, nullptr, &nothing);
    if (s != OV2_OK || nothing) return s;
    if ((s = ov2_match_to_map_batch_dev(c, &in, fmaxprojerr, fdistratio, X.work, X.match_cand, X.match_dist)) != OV2_OK) return s;
    out->d_kp_off = in.kp_off; out->d_cand_off = in.cand_off; out->d_kp_lmid = dkp; out->d_cand_lmid = dcand;
    out->d_match_cand = X.match_cand; out->d_match_dist = X.match_dist;
    if (pairs) {
        if ((s = ov2_match_pairs_dev(c, B, in.n_kp, in.kp_off, in.cand_off, dkp, dcand, X.match_cand, X.prev_lmid, X.new_lmid, X.n_pairs)) != OV2_OK)
            return s;
        out->d_prev_lmid = X.prev_lmid; out->d_new_lmid = X.new_lmid; out->d_n_pairs = X.n_pairs;
    }
    return OV2_OK;
}

extern "C" ov2_status ov2_map_match_local_batch(ov2_ctx *c, int B, ov2_map *const *maps, const int32_t *newkf, const int32_t *nb3dkps,
                                                const int32_t *kp_off, const int32_t *kp_lmid, const int32_t *grid_ptr,
                                                const int32_t *grid_kp, const int32_t *cand_off, const int32_t *cand_lmid,
                                                const double *K, int img_w, int img_h, int cell, const ov2_cam_model *cam,
                                                float fmaxprojerr, float fdistratio, int32_t *match_lmid, float *match_dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (B > 0 && kp_off && kp_off[0] == 0 && kp_off[B] > 0 && (!match_lmid || !match_dist))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_match_local_batch: null output");
    ov2_match_batch_input in;
    gather_extra X;
    bool nothing;
    unsigned char *res = nullptr;
    const size_t res_bytes = (B > 0 && kp_off && kp_off[B] > 0) ? 2 * (((size_t)kp_off[B] * 4 + 255) & ~(size_t)255) : 0;
    ov2_status s = gather_impl(c, "ov2_map_match_local_batch",
                               gather_args_of(B, maps, newkf, nb3dkps, kp_off, kp_lmid, grid_ptr, grid_kp, cand_off, cand_lmid, K, img_w, img_h, cell, cam),
                               &in, nullptr, nullptr, &X, res_bytes, &res, &nothing);
    if (s != OV2_OK || nothing) return s;
    if ((s = ov2_match_to_map_batch_dev(c, &in, fmaxprojerr, fdistratio, X.work, X.match_cand, X.match_dist)) != OV2_OK) return s;
    // match_cand and match_dist lie behind each other in the scratch block (each padded to 256 bytes): one download
    const size_t n = (size_t)in.n_kp, stride = (n * 4 + 255) & ~(size_t)255;
    OV2_HIP(c, hipMemcpyAsync(res, X.match_cand, stride + n * 4, hipMemcpyDeviceToHost, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t *mc = (const int32_t *)res;
    memcpy(match_dist, res + stride, n * 4);
    for (int b = 0; b < B; ++b) {
        const int nc = cand_off[b + 1] - cand_off[b];
        for (int k = kp_off[b]; k < kp_off[b + 1]; ++k)
            match_lmid[k] = (mc[k] >= 0 && mc[k] < nc) ? cand_lmid[cand_off[b] + mc[k]] : -1;
    }
    return OV2_OK;
}

// ---- saved state (bench / tests: every job starts from the same map) ----------------------------------------------
extern "C" ov2_status ov2_map_save_state(ov2_map *m)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    OV2_HIP(c, hipSetDevice(c->device));
    void *old[] = {m->snap_kf_pose, m->snap_lm_xyz, m->snap_kf_state, m->snap_lm_state, m->snap_obs_flag};
    for (void *p : old) if (p) (void)hipFree(p);
    m->snap_kf_pose = m->snap_lm_xyz = nullptr; m->snap_kf_state = m->snap_lm_state = m->snap_obs_flag = nullptr;
    const size_t K = m->max_kf, L = m->max_lm, N = m->n_obs;
    ov2_status s = OV2_OK;
    if (s == OV2_OK) s = dmalloc(c, &m->snap_kf_pose, 7 * K);
    if (s == OV2_OK) s = dmalloc(c, &m->snap_lm_xyz, 3 * L);
    if (s == OV2_OK) s = dmalloc(c, &m->snap_kf_state, K);
    if (s == OV2_OK) s = dmalloc(c, &m->snap_lm_state, L);
    if (s == OV2_OK) s = dmalloc(c, &m->snap_obs_flag, N);
    if (s != OV2_OK) return s;
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(m->snap_kf_pose, m->kf_pose, 7 * K * 8, hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemcpyAsync(m->snap_lm_xyz, m->lm_xyz, 3 * L * 8, hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemcpyAsync(m->snap_kf_state, m->kf_state, K, hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipMemcpyAsync(m->snap_lm_state, m->lm_state, L, hipMemcpyDeviceToDevice, st));
    if (N) OV2_HIP(c, hipMemcpyAsync(m->snap_obs_flag, m->obs_flag, N, hipMemcpyDeviceToDevice, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    m->snap_kf = (int)K; m->snap_lm = (int)L; m->snap_obs = (int)N; m->snap_floor = 0;
    free(m->snap_kf_alive_h);
    if (!(m->snap_kf_alive_h = (unsigned char *)malloc(std::max<size_t>(K, 1)))) return ov2_set_err(c, OV2_ERR_NOMEM, "saved keyframe list");
    memcpy(m->snap_kf_alive_h, m->kf_alive_h, K);
    return OV2_OK;
}

extern "C" ov2_status ov2_map_restore_state_batch(ov2_ctx *c, int B, ov2_map *const *maps)
{
    if (!c) return OV2_ERR_INVALID;
    if (B == 0) return OV2_OK;
    if (B < 0 || !maps) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_restore_state_batch: null argument");
    ov2_status s;
    for (int b = 0; b < B; ++b) {
        ov2_map *m = maps[b];
        if ((s = batch_map_ok(c, m, b)) != OV2_OK) return s;
        if (!m->snap_kf_pose || m->snap_kf != m->max_kf || m->snap_lm != m->max_lm || m->snap_obs != m->n_obs)
            return ov2_set_err(c, OV2_ERR_INVALID, "map %d: no saved state, or the tables changed shape since it was saved", b);
    }
    OV2_HIP(c, hipSetDevice(c->device));
    job_table JT;
    if ((s = JT.begin(c, B)) != OV2_OK) return s;
    for (int b = 0; b < B; ++b) {
        JT.set(b, job_of(maps[b], -1, -1)); maps[b]->last_valid = 0;
        // a keyframe the restore takes out of the map (one that entered after the save) loses its local id set like any
        // removed keyframe; the sets of the others are not part of the saved state and stay
        for (int k = 0; maps[b]->ls_on && k < maps[b]->max_kf; ++k)
            if (maps[b]->kf_alive_h[k] && !maps[b]->snap_kf_alive_h[k] && (s = ls_forget(maps[b], k)) != OV2_OK) return s;
        memcpy(maps[b]->kf_alive_h, maps[b]->snap_kf_alive_h, (size_t)maps[b]->max_kf);
    }
    if ((s = JT.upload()) != OV2_OK) return s;
    OV2_LAUNCH(c, OV2_K_MAP, mb_restore_kernel, dim3(64, B), dim3(256), 0, c->stream, JT.dev);
    // the job table must have been read before the staging block is reused: the next call that stages waits for this
    // stream anyway (same stream, in order), and a staging reallocation synchronises first
    return OV2_OK;
}

// ---- the tables to host memory (tests) ----------------------------------------------------------------------------
extern "C" ov2_status ov2_map_download(ov2_map *m, int *n_kf, int *n_lm, int *n_obs, double *kf_pose, uint8_t *kf_state, double *lm_xyz,
                                       uint8_t *lm_state, int32_t *obs_kf, int32_t *obs_lm, uint8_t *obs_flag, double *obs_uv, double *obs_ruv)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    if (n_kf) *n_kf = m->max_kf;
    if (n_lm) *n_lm = m->max_lm;
    if (n_obs) *n_obs = m->n_obs;
    const size_t K = m->max_kf, L = m->max_lm, N = m->n_obs;
#define DL(dst, src, bytes) if ((dst) && (bytes)) OV2_HIP(c, hipMemcpy((dst), (src), (bytes), hipMemcpyDeviceToHost))
    DL(kf_pose, m->kf_pose, 7 * K * 8); DL(kf_state, m->kf_state, K); DL(lm_xyz, m->lm_xyz, 3 * L * 8); DL(lm_state, m->lm_state, L);
    DL(obs_kf, m->obs_kf, N * 4); DL(obs_lm, m->obs_lm, N * 4); DL(obs_flag, m->obs_flag, N); DL(obs_uv, m->obs_uv, 2 * N * 8);
    DL(obs_ruv, m->obs_ruv, 2 * N * 8);
#undef DL
    return OV2_OK;
}

extern "C" ov2_status ov2_map_download_match_columns(ov2_map *m, float *obs_px, uint8_t *obs_desc, uint8_t *obs_hasdesc)
{
    if (!m || !m->c) return OV2_ERR_INVALID;
    ov2_ctx *c = m->c;
    if (!m->obs_hasdesc) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_map_download_match_columns: the map has no match columns");
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    const size_t N = m->n_obs;
    if (obs_px && N) OV2_HIP(c, hipMemcpy(obs_px, m->obs_px, 2 * N * sizeof(float), hipMemcpyDeviceToHost));
    if (obs_desc && N) OV2_HIP(c, hipMemcpy(obs_desc, m->obs_desc, 32 * N, hipMemcpyDeviceToHost));
    if (obs_hasdesc && N) OV2_HIP(c, hipMemcpy(obs_hasdesc, m->obs_hasdesc, N, hipMemcpyDeviceToHost));
    return OV2_OK;
}
