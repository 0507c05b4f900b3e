// ov2_slam.hpp -- the per-frame / per-keyframe drivers of the reference on top of the host mirror (ov2_host.hpp), so that
// a closed loop runs through C++ and the C ABI without Python in the path:
//   MotionModel                      include/visual_front_end.hpp:38-90
//   VisualFrontEnd::visualTracking   src/visual_front_end.cpp:40-62        trackMono :66-130      checkNewKfReq :985-1064
//                   computeParallax  :1069-1142
//   MapManager::createKeyframe       src/map_manager.cpp:43-60  prepareFrame :64-115  extractKeypoints :286-340
//               addKeypointsToFrame  :196-211   addKeyframe :621-634   addMapPoint :636-659
//   Mapper::run (one keyframe)       src/mapper.cpp:38-189      triangulateStereo :346-461   triangulateTemporal :191-344
//                   matchingToLocalMap :469-554  matchToMap :576-774 (ov2_match_to_map; B keyframes of B maps at once:
//                   SlamManager::matchToLocalMaps on ov2_match_to_map_batch)
//   SlamManager::run (one image)     src/ov2slam.cpp:152-205    Estimator::applyLocalBA  src/estimator.cpp:67-98
// The reference runs front-end, mapper and estimator on three threads; here one call processes one stereo frame to the
// end (keyframe work included), i.e. the reference with bforce_realtime = 0 and an idle back-end: deterministic.
// VisualFrontEnd::epipolar2d2dFiltering :446-655 runs with doepipolar_ (ov2_epipolar_filter_batch); computePose runs its
// P3P-LMedS bootstrap (ov2_p3p_ransac_batch) when tracking asks for it (bp3preq_) or dop3p_ is set, and resetFrame() where
// that fails.
//   LoopCloser (2D-2D half)         src/loop_closer.cpp:184-236  knnMatching :378-459  epipolarFiltering :462-499
//                                   removeOutliers :899-928
//   LoopCloser::trackLoopLocalMap   src/loop_closer.cpp:502-583  matchToMap :586-763 (ov2_loop_match_to_map_batch)
//               computePnP          :834-897
// Out of scope and refused loudly where reached: the mono branch of the epipolar filter.  Of loop closing, what decides
// whether a candidate keyframe is a loop is built up to the pair list that p3pRansac would receive, and from the pose it
// returns through trackLoopLocalMap and computePnP to the accepted pose and pair list (LoopCloser below); the frame loop calls
// none of it, because nothing proposes candidates yet.
#pragma once
#include "ov2_host.hpp"
#include "ov2_lcd.hpp"

namespace ov2 {

// Knobs that replace three heuristics of the reference by the fixed stand-ins of ov2slam_amd/slam_loop.py, so that this
// driver can be compared pose by pose with that loop (and through it with the CPU oracle); all zero = the reference.
struct LoopPolicy {
    int kf_every = 0;             // > 0: a keyframe every kf_every-th frame instead of checkNewKfReq
    int ba_window = 0;            // > 0: local BA over the last ba_window keyframes (the oldest ba_fixed constant) instead of the covisibility walk
    int ba_fixed = 2;
    bool compose_motion = false;  // prediction = Twc * (Twc_prev^-1 * Twc) instead of exp(log(.) / dt * dt) (equal up to rounding)
    bool midpoint_stereo = false; // stereo triangulation by the mid-point method also for rectified rigs; a failed triangulation
                                  // keeps the stereo observation (the reference demotes it, src/mapper.cpp:412,428,440)
    bool pose_from_kf = false;    // after a local BA the current frame takes the refined pose of its keyframe
};

class MotionModel {   // include/visual_front_end.hpp:38-90: constant velocity in se3
public:
    void applyMotionModel(SE3 &Twc, double time);
    void updateMotionModel(const SE3 &Twc, double time);
    void reset() { prev_time_ = -1.; for (double &v : log_relT_) v = 0.; }
    double prev_time_ = -1.;
    SE3 prevTwc_;
    double log_relT_[6] = {0, 0, 0, 0, 0, 0};   // [upsilon, omega] per second
};

void se3_log(const SE3 &T, double out[6]);   // Sophus::SE3::log  (se3.hpp), tangent order [upsilon, omega]
SE3 se3_exp(const double a[6]);              // Sophus::SE3::exp  (se3.hpp:763-784)

struct Keyframe {   // include/mapper.hpp:39-85: what the front-end hands to the mapper
    int kfid_ = -1;
    Pyramid vpyr_imleft_;
    const uint8_t *imrightraw_ = nullptr;
    int w = 0, h = 0, stride = 0;
};

struct SlamStats {   // per frame, for tests / profiles
    int frame = 0, tracked = 0, n3d = 0, is_kf = 0, n_new = 0, n_stereo = 0, n_lm3d = 0;
    int ba_done = 0, ba_res = 0, ba_it_robust = 0, ba_it_l2 = 0, ba_outliers = 0;
    int n_described = 0, n_local = 0, n_matched = 0;   // keyframe: keypoints with a descriptor, local map points offered, merges
    double ba_cost0 = 0., ba_cost1 = 0.;
};

// One Mapper::matchToMap call (src/mapper.cpp:576-774) taken apart: what the reference's loops look at as the flat arrays of
// ov2_match_input (SlamManager::assembleMatchToMap fills them), and what its result means for the map.
struct MatchJob {
    // in: the map, and for SlamManager::matchToLocalMaps the keyframe and the local map points offered (the iteration order of
    // the set decides ties)
    MapManager *pmap = nullptr;
    int kfid = -1;
    std::unordered_set<int> set_local_lmids;
    // assembled: kp_lmid / cand_lmid name the rows; offered = false when there is nothing to match (an empty local set, no
    // keypoint or no candidate): such a job takes no slot in a call
    bool offered = false;
    std::vector<int> kp_lmid, cand_lmid;
    double Twc[7] = {0}, K[4] = {0};
    int img_w = 0, img_h = 0, cell = 0, nb3dkps = 0;
    bool distorted = false;
    ov2_cam_model cam{};
    std::vector<float> kp_px, kp_kf_px;
    std::vector<int32_t> kp_desc_ptr, kp_kf_ptr, kp_kfids, grid_ptr, grid_kp, cand_desc_ptr, cand_kf_ptr, cand_kfids;
    std::vector<uint8_t> kp_descs, cand_descs;
    std::vector<double> cand_wpt, kf_Twc;
    // out: keypoint lmid -> local map point id (the reference's map_previd_newid)
    std::map<int, int> map_previd_newid;
};

struct MatchBatchStats {   // one matchToLocalMaps call
    int jobs = 0, match_jobs = 0;      // jobs given, jobs with something to offer
    int n_kp = 0, n_cand = 0;          // keypoints and candidates offered over all jobs
    int match_calls = 0;               // library calls made: 0 or 1 batched, one per offered job with `single`
};

class SlamManager {   // src/ov2slam.cpp (the stereo branch of run())
public:
    SlamManager(ov2_ctx *ctx, std::shared_ptr<SlamParams> pstate, std::shared_ptr<CameraCalibration> cl,
                std::shared_ptr<CameraCalibration> cr, const LoopPolicy &policy);
    // one stereo frame through visualTracking and, when it asks for a keyframe, Mapper::run + Estimator::applyLocalBA
    // followed by Estimator::mapFiltering (src/estimator.cpp:45-47; off while SlamParams::fkf_filtering_ratio_ is 1)
    ov2_status addNewStereoImages(double time, const uint8_t *im0, const uint8_t *im1, int w, int h, int stride);
    SE3 pose() const { return pcurframe_->getTwc(); }
    // the 256 test pairs of BRIEF-32 (y1, x1, y2, x2 per test, int8: opencv_contrib's generated_32.i, absent from the reference
    // tree, so the caller supplies it) -- with use_brief_ the keyframe path describes its keypoints and runs
    // Mapper::matchingToLocalMap (src/mapper.cpp:469-554)
    void setBriefPattern(const int8_t *pattern256x4) { brief_pattern_.assign(pattern256x4, pattern256x4 + 1024); }
    std::vector<int8_t> brief_pattern_;

    ov2_ctx *ctx_;
    std::shared_ptr<SlamParams> pslamstate_;
    std::shared_ptr<Frame> pcurframe_;
    std::shared_ptr<MapManager> pmap_;
    std::shared_ptr<FeatureTracker> ptracker_;
    std::shared_ptr<FeatureExtractor> pfeatextract_;
    std::shared_ptr<VisualFrontEnd> pvisualfrontend_;
    std::shared_ptr<Optimizer> poptimizer_;
    std::shared_ptr<Estimator> pestimator_;
    LoopPolicy policy_;
    MotionModel motion_model_;
    int frame_id_ = -1;
    SlamStats last_;
    EpiStats last_epi_;   // epipolar2d2dFiltering on the last frame (doepipolar_)
    P3pStats last_p3p_;   // the P3P branch of computePose on the last frame (bp3preq_ or dop3p_)
    TemporalStats last_temporal_;   // triangulateTemporal on the last keyframe (do_temporal_)
    // Mapper::triangulateTemporal (src/mapper.cpp:191-344): the 2D keypoints of a new keyframe whose map point an older keyframe
    // observes turn 3D once the two views triangulate them (a keypoint whose stereo match failed stays 2D for good without it).
    // Mapper::run calls it for every keyframe with nb2dkps_ > 0 && kfid_ > 0, stereo as well as mono (:107-126); mapperRun does
    // so only with SlamParams::do_temporal_, which the reference does not have and which is OFF by default: the existing loop
    // tests hold exact counts recorded without the stage.  Selection and bookkeeping run here, the per-pair arithmetic is one
    // ov2_triangulate_pairs call over all source keyframes.  Static so that a bare MapManager (tests) can run it too.
    static ov2_status triangulateTemporal(ov2_ctx *ctx, MapManager &map, const SlamParams &st, Frame &frame, TemporalStats &stats);
    // Mapper::triangulateStereo (src/mapper.cpp:346-461): the stereo keypoints of a new keyframe that are not 3D yet.  Selection
    // and bookkeeping run here, the per-pair arithmetic is one ov2_triangulate_pairs call (mid-point, or the disparity form with
    // SlamParams::bdo_stereo_rect_ unless midpoint_always).  demote: a failed keypoint loses its stereo flag, as in the
    // reference (LoopPolicy::midpoint_stereo keeps it).  Static so that a bare MapManager (tests) can run it too;
    // ov2_map_triangulate_stereo_batch is its mirror form.
    static ov2_status triangulateStereo(ov2_ctx *ctx, MapManager &map, const SlamParams &st, Frame &frame, StereoTriStats &stats,
                                        bool midpoint_always = false, bool demote = true);
    // Mapper::matchToMap (src/mapper.cpp:576-774) in three parts.  assembleMatchToMap reads job.pmap, `frame` and the local set and fills the flat
    // arrays (no GPU context needed); the library call is ov2_match_to_map on matchInput(job), or ov2_match_to_map_batch on several
    // jobs at once; applyMatches turns match_cand (one entry per keypoint of the job) into job.map_previd_newid.
    static void assembleMatchToMap(const Frame &frame, const std::unordered_set<int> &set_local_lmids, MatchJob &job);
    static void matchInput(const MatchJob &job, ov2_match_input &in);
    static void applyMatches(MatchJob &job, const int32_t *match_cand);
    // The re-matching of B new keyframes against their local maps -- distinct maps that share `ctx` --: assemble every job, ONE
    // ov2_match_to_map_batch call whatever B is (none when no job has anything to offer), apply per job and, with `merge`,
    // MapManager::mergeMapPoints per pair (Mapper::mergeMatches, :556-574).  A job whose keyframe is not in its map, or a camera
    // that differs among the offered jobs (the call takes one), is OV2_ERR_INVALID before anything is enqueued.  single: the same
    // jobs as one ov2_match_to_map call each, the shape of the per-keyframe path.
    // mirror (off by default): when every job's map has a device mirror with the match columns (MapManager::enableMatchColumns),
    // the maps are flushed and the call is ov2_map_match_local_batch on the mirrors -- only ids go up: the keypoints' lmids in
    // grid order, the grid, the local set unfiltered in its iteration order (n_cand then counts the unfiltered ids).  Otherwise
    // the flag is ignored.
    static ov2_status matchToLocalMaps(ov2_ctx *ctx, std::vector<MatchJob> &jobs, float fmaxprojerr, float fdistratio, bool merge, bool single,
                                       MatchBatchStats &stats, bool mirror = false);
    // The set assembly of Mapper::matchingToLocalMap (src/mapper.cpp:475-517), what it does in front of matchToMap: with an
    // empty covisibility map nothing happens (the reference dereferences begin() of an empty map); otherwise, when the
    // frame's local set holds fewer than nmax_localplms ids, the stored set of the oldest covisible keyframe joins it (a
    // keyframe that left the map: the next older one that is there, :485-488).  Returns whether that branch was taken.
    // Static so that a bare MapManager (tests) can run it too; ov2_map_local_ids_batch is its mirror form.
    static bool extendLocalMap(MapManager &map, Frame &frame, size_t nmax_localplms);
    // the ids of a job for the mirror path: kp_lmid / grid as assembleMatchToMap lists them, cand_lmid = the local set as it iterates
    static void assembleMatchIds(const Frame &frame, const std::unordered_set<int> &set_local_lmids, MatchJob &job);
    std::vector<SlamStats> stats_;
    std::vector<SE3> traj_;

private:
    bool visualTracking(const uint8_t *iml, int w, int h, int stride, double time, ov2_status *st);   // :40-62
    bool trackMono(const uint8_t *im, int w, int h, int stride, double time, ov2_status *st);          // :66-130
    bool checkNewKfReq();                                                                              // :985-1064
    float computeParallax(int kfid, bool do_unrot, bool bmedian, bool b2donly);                        // :1069-1142
    ov2_status createKeyframe();                                                                       // src/map_manager.cpp:43-60
    void prepareFrame();
    ov2_status extractKeypoints();
    void addKeypointsToFrame(const std::vector<Point2f> &vpts, Frame &frame);
    void addKeypointsToFrame(const std::vector<Point2f> &vpts, const std::vector<Desc> &vdescs, const std::vector<uint8_t> &valid, Frame &frame);
    ov2_status describeBRIEF(const std::vector<Point2f> &vpts, std::vector<Desc> &vdescs, std::vector<uint8_t> &valid);   // src/feature_extractor.cpp:224-285
    ov2_status describeKeypoints(const std::vector<Keypoint> &vkps, const std::vector<Point2f> &vpts);                   // src/map_manager.cpp:343-362
    ov2_status matchingToLocalMap(Frame &frame);                                                        // src/mapper.cpp:469-554
    ov2_status matchToMap(const Frame &frame, float fmaxprojerr, float fdistratio, std::unordered_set<int> &set_local_lmids,
                          std::map<int, int> &map_previd_newid);                                        // :576-774 -> ov2_match_to_map
    Pyramid raw_pyr_;        // level 0 of the raw left image (describeBRIEF works on imraw, src/map_manager.cpp:300, 325)
    const uint8_t *imraw_ = nullptr; int imw_ = 0, imh_ = 0, imstride_ = 0;
    void addKeyframe();
    ov2_status mapperRun(const Keyframe &kf);                                                          // src/mapper.cpp:38-189
    ov2_status triangulateStereo(Frame &frame)                                                         // :346-461
    {
        StereoTriStats ts;
        return triangulateStereo(ctx_, *pmap_, *pslamstate_, frame, ts, policy_.midpoint_stereo, !policy_.midpoint_stereo);
    }
    ov2_status triangulateTemporal(Frame &frame) { return triangulateTemporal(ctx_, *pmap_, *pslamstate_, frame, last_temporal_); }   // :191-344
    ov2_status fixedWindowBA();                                                                        // LoopPolicy::ba_window
    int nkfid_ = 0, nlmid_ = 0;
    SE3 Twc_prev_;           // compose_motion: the pose of the frame before the last
    bool have_prev_ = false;
};

// what LoopCloser::processLoopCandidate did with one candidate pair, up to the call of p3pRansac (src/loop_closer.cpp:201-236)
enum LoopBranch {
    LC_COVISIBLE = 0,     // :201-209 covisibility score > 30
    LC_FEW_MATCHES,       // :217 fewer than 15 pairs after knnMatching
    LC_FILTER_FAILED,     // :227 the 5-point RANSAC failed or left fewer than 10 inliers
    LC_PASSED             // :233-236 the pair list p3pRansac would receive
};

struct LoopKnnInputs {   // what knnMatching assembles for one pair (:380-424), in the mirror's iteration order
    std::vector<std::pair<int, int>> vkplmids;   // identity pairs (:393-395)
    std::vector<int> vkpids, vlmids;             // lmid of every query / train row
    std::vector<uint8_t> query, train;           // rows x 32
};

struct LoopPairResult {
    int lckfid = -1;                                  // the candidate used (:192-195 walk down to a keyframe still in the map)
    int branch = LC_COVISIBLE;
    int n_identity = 0, n_query = 0, n_train = 0;     // rows of n_query / n_train are 0 when the pair did not reach the matcher
    std::vector<std::pair<int, int>> vkplmids_knn;    // after knnMatching (empty for LC_COVISIBLE)
    std::vector<std::pair<int, int>> vkplmids;        // after removeOutliers (LC_PASSED only)
    int epi_status = -1;                              // -1: not offered to the filter; else the ov2_epipolar_filter_batch status
    int epi_info[4] = {0, 0, -1, 0};                  // its info: iterations, skipped draws, chosen draw, inlier count
    int n_outliers = 0;                               // voutliers_idx.size() (0 unless the filter returned true)
    double R[9] = {0}, t[3] = {0};                    // [R12 | t12] of the filter where epi_status >= 1
};

struct LoopStats {   // one matchLoopCandidates call
    int pairs = 0, knn_pairs = 0, epi_pairs = 0;   // pairs given, offered to the matcher, offered to the 5-point filter
    int knn_calls = 0, epi_calls = 0;              // launches of each (0 or 1)
    // verifyLoopCandidates (zero after matchLoopCandidates alone): pairs that reached P3P, the refinement, the local-map matcher
    // and computePnP, and the library calls made for each stage (0 or 1 whatever B is)
    int p3p_pairs = 0, refine_pairs = 0, track_pairs = 0, pnp_pairs = 0;
    int p3p_calls = 0, refine_calls = 0, track_calls = 0, pnp_calls = 0;
};

// what the 2D-3D half of LoopCloser::processLoopCandidate did with one pair (src/loop_closer.cpp:238-300); an enum of its own,
// LoopBranch and LoopPairResult keep their meaning
enum LoopVerifyBranch {
    LV_P3P_FAILED = 0,    // :251 p3pRansac false (fewer than 4 pairs, no model) or fewer than 5 inliers
    LV_NO_NEW_MATCHES,    // :275, :298-300 trackLoopLocalMap added nothing
    LV_PNP_FAILED,        // :288 computePnP false or fewer than 30 inliers
    LV_FEW_GOOD,          // :305 fewer than 30 pairs left
    LV_ACCEPTED           // the loop would be closed: Twc and vkplmids are what localPoseGraph / mergeMapPoints receive
};

struct LoopVerifyResult {
    int branch = LV_P3P_FAILED;
    int p3p_status = -1;                          // -1: P3P not run (fewer than 4 pairs); else the ov2_p3p_ransac_batch status
    int p3p_info[4] = {0, 0, -1, 0};              // its info: counted draws, skipped draws, chosen draw, inliers
    std::vector<std::pair<int, int>> vkplmids_p3p, vkplmids_track, vkplmids;   // after P3P + removeOutliers, after tracking, at the end
    std::vector<int> pnp_outliers;                // computePnP's voutliers_idx (indices into vkplmids_track)
    int n_identity = 0, n_offered = 0, n_matched = 0;
    SE3 Twc_p3p, Twc;                             // after P3P + refinement; after computePnP
    double lc_pose_err = 0.;                      // :318 |log(Tcw_new * Twc)|
};

struct LoopLocalMap {   // what trackLoopLocalMap assembles in front of its matcher (:502-568 and the candidate filter of :612-631)
    int n_identity = 0;                 // identity pairs appended to vkplmids (:543-548)
    std::vector<int> vmatchedkpids;     // first elements of vkplmids after those additions (:559-561)
    std::vector<int> vlocal;            // set_local_lmids without the second elements of vkplmids (:562), ORDER OF FIRST ENCOUNTER
    std::vector<int> vcands;            // vlocal after the candidate filter (:614-631), same order: what the matcher is offered
};

struct LoopTrackJob {   // one trackLoopLocalMap call (:269): in: the pair, the projection pose (the P3P result), vkplmids
    int newkfid = -1, lckfid = -1;
    SE3 Twc;
    std::vector<std::pair<int, int>> vkplmids;   // in / out
    int n_identity = 0, n_offered = 0, n_matched = 0;   // out: identity pairs appended, candidates offered, matches appended
};

struct LoopTrackStats {   // one trackLoopLocalMaps call
    int pairs = 0, match_pairs = 0, match_calls = 0;   // jobs given, offered to the matcher, launches of it (0 or 1)
};

// The 2D-2D half of LoopCloser::processLoopCandidate (src/loop_closer.cpp:184-236): does the new keyframe see the same place
// as a candidate keyframe?  The second half (:238-300) decides it: p3pRansac with a refinement, trackLoopLocalMap, computePnP,
// for one pair as the reference writes it (verifyLoopCandidate) and for B pairs with one library call per stage
// (verifyLoopCandidates).  newKeyframe is the body of LoopCloser::run for one keyframe (:86-169): the detector that proposes the
// candidate (ov2::LCDetector, ov2_lcd.hpp) in front of processLoopCandidates; with the keyframe's raw image it also detects and
// describes the 300 extra FAST + BRIEF keypoints of :115-140 (extraKeypoints) and hands the detector both sets.  closeLoop is
// what follows an accepted loop (:302-372): localPoseGraph, mergeMapPoints, structureOnlyBA, looseBA; closeLoops does it for
// the loops of B maps with one pose-graph solve call.  With close_loops_ set, newKeyframe(s) go on to it; it is off by default.
// Not built: any call from SlamManager's frame loop.
// what LoopCloser::closeLoop did with an accepted loop (src/loop_closer.cpp:302-372)
enum LoopCloseBranch {
    LCL_FEW_PAIRS = 0,     // :305 fewer than 30 pairs: nothing is called
    LCL_PG_REFUSED,        // :320 localPoseGraph returned false (no chain, or the degenerate test of src/optimizer.cpp:2467-2474): the map is untouched
    LCL_CLOSED,            // pose graph applied, pairs merged, structureOnlyBA run; lc_pose_err < 0.02: no looseBA
    LCL_CLOSED_LOOSE_BA    // ... and looseBA run (:358-371)
};
enum { LCL_NOT_CALLED = 1 };   // value of a status field whose call was not made (an ov2_status is <= 0)

struct LoopCloseResult {
    int branch = LCL_FEW_PAIRS;
    int inikfid = -1;                 // :314 the smallest key of the loop keyframe's covisibility map
    int loose_start = -1;             // :363 the smallest key of inikf's covisibility map (looseBA's first keyframe)
    double lc_pose_err = 0.;          // :318
    int pg_status = LCL_NOT_CALLED;   // status of the pose-graph solve
    ov2_pg_result pg{};
    std::vector<int> vmergedlmids;    // :347 the new lmid of every pair with prev != new, in list order
    int sba_status = LCL_NOT_CALLED, loose_status = LCL_NOT_CALLED;   // structureOnlyBA (:353), looseBA (:368)
};

class LoopCloser;

struct LoopCloseJob {   // one accepted loop for LoopCloser::closeLoops
    LoopCloser *closer = nullptr;
    int newkfid = -1, lckfid = -1;
    SE3 Twc;
    std::vector<std::pair<int, int>> vkplmids;
    LoopCloseResult r;   // out
};

struct LoopCloseStats {   // one closeLoop(s) call
    int jobs = 0, graphs = 0, solve_calls = 0;   // jobs given, graphs offered to ov2_pose_graph_solve_batch, calls of it (0 or 1)
};

struct LoopNewKeyframeResult {
    bool skipped = false;        // :111-113 no map point of the keyframe has a descriptor: the detector is not called
    int image_id = -1;           // kf_idx_ of this keyframe (index into vkfids_); -1 when skipped
    LCDetectorResult det;        // the detector's result (status LC_NOT_DETECTED when skipped)
    int cand_kfid = -1;          // on LC_DETECTED: vkfids_[train_id], walked down to the closest keyframe still in the map (:187-195)
    LoopPairResult matched;      // processLoopCandidates on (kfid, cand_kfid); untouched without a candidate
    LoopVerifyResult verified;
    LoopCloseResult closed;      // closeLoop on an LV_ACCEPTED result while close_loops_ is set; untouched otherwise
    int nbkps = 0, n_extra = 0;  // the two counts the reference logs (:138): vkps.size() and vaddkps.size(); image forms only
    int n_descs = 0;             // descriptor rows the detector received
};

class LoopCloser;

struct LoopExtraJob {   // one (keyframe, raw image) pair of LoopCloser::extraKeypoints
    LoopCloser *closer = nullptr;
    int kfid = -1;
    int b = 0;                           // image of the pyramid batch
    // out
    bool skipped = false;                // :111-113 no map point of the keyframe has a descriptor: nothing detected for it
    int nbkps = 0;                       // vkps.size() (:90)
    std::vector<uint8_t> map_descs;      // plm->desc_ of the keypoints whose map point exists and has one (:97-109), rows of 32
    std::vector<Point2f> mask_px;        // kp.px_ of exactly those keypoints: the centres of the mask discs (:107)
    int n_detected = 0;                  // keypoints after retainBest (:126)
    std::vector<Point2f> add_px;         // the ones BRIEF describes (28 px or more from the border, :129), row-major
    std::vector<uint8_t> add_resp;
    std::vector<uint8_t> add_descs;      // rows of 32
};

struct LoopExtraStats {   // library calls of one extraKeypoints
    int detect_calls = 0, describe_calls = 0;
};

class LoopCloser {
public:
    LoopCloser(ov2_ctx *ctx, std::shared_ptr<SlamParams> pstate, std::shared_ptr<MapManager> pmap)
        : ctx_(ctx), pslamstate_(pstate), pmap_(pmap) {}
    // :86-169 for one keyframe of the map: the descriptors (plm->desc_) of the keyframe's keypoints whose map point exists and
    // has one, in getKeypoints() order; none: skipped, the image id does not advance.  Otherwise kfid goes to vkfids_ and the
    // detector processes image kf_idx_; on LC_DETECTED train_id is mapped through vkfids_ (walking down while the keyframe is no
    // longer in the map; below keyframe 0 there is no candidate, where the reference would not end) and the pair goes to
    // processLoopCandidates.  The detector is created on first use with lcd_params_ on this closer's context.
    ov2_status newKeyframe(int kfid, uint64_t seed, LoopNewKeyframeResult &r);
    // :95-134 for B (keyframe, image b of `pyr`) pairs, `pyr` = level 0 of the RAW left images (built without CLAHE): the mask
    // discs of radius 2 around the described keypoints, whole-image FAST(20) with non-maximum suppression, retainBest(300) and
    // BRIEF on the raw image with the pattern of the first job's closer -- ONE ov2_fast_detect_batch call and ONE
    // ov2_describe_brief_batch call whatever B is (none for the jobs that are skipped, which comes before detection, :111-113).
    // The detect call has room for extra_out_cap_ keypoints per image; if an image has more, it is repeated once with room for
    // the largest.  Keypoints without a descriptor (border) are dropped after retainBest, as compute does.  Images of the batch
    // that no job names are detected on without a mask and ignored; two jobs on one image are OV2_ERR_INVALID.
    static ov2_status extraKeypoints(ov2_ctx *ctx, const ov2_pyr *pyr, std::vector<LoopExtraJob> &jobs, LoopExtraStats &stats);
    // newKeyframe with the keyframe's raw image: the same, with the extra descriptors appended behind the map points' (:131-134)
    ov2_status newKeyframe(int kfid, uint64_t seed, const ov2_pyr *pyr, int b, LoopNewKeyframeResult &r);
    // the step for B closers (distinct, on one context) and one keyframe each: one extraKeypoints, then LCDetector::processBatch
    // over the closers that were not skipped, then processLoopCandidates for each closer whose detector proposed a candidate
    static ov2_status newKeyframes(const std::vector<LoopCloser *> &closers, const std::vector<int> &kfids, const std::vector<uint64_t> &seeds,
                                   const ov2_pyr *pyr, const std::vector<int> &bs, std::vector<LoopNewKeyframeResult> &out,
                                   LoopExtraStats *stats = nullptr);
    // the 256 test pairs of BRIEF-32, as SlamManager::setBriefPattern
    void setBriefPattern(const int8_t *pattern256x4) { brief_pattern_.assign(pattern256x4, pattern256x4 + 1024); }
    std::vector<int8_t> brief_pattern_;
    int extra_fast_th_ = 20, extra_mask_radius_ = 2, extra_nbest_ = 300;   // :107, :123 (pfastd_ = FastFeatureDetector::create(20)), :126
    int extra_out_cap_ = 2048;
    LoopExtraStats last_extra_;   // of the last image-form newKeyframe(s) this closer took part in
    LCDetectorParams lcd_params_;
    std::unique_ptr<LCDetector> plcdetector_;
    std::vector<int> vkfids_;
    int kf_idx_ = -1;
    // :502-568 + :612-631, the part of trackLoopLocalMap in front of the matcher (no GPU): the candidate's covisible keyframes in
    // ascending id with the candidate forced in, the window lckf.kfid_ +- 15 (`continue` below it, `break` above it), keyframes
    // no longer in the map skipped, every lmid looked at once; an lmid the new keyframe observes becomes an identity pair
    // (appended to vkplmids unless that pair is already there), the others form the local set, minus the second elements of
    // vkplmids; then the filter the matcher applies before it projects: observed by the frame, gone, not 3D, isBad() (called
    // as the reference calls it: it may clear is3d_), no descriptor.  The reference keeps the local set in an unordered_set,
    // so the order in which it offers the candidates is implementation-defined; here it is a vector in ORDER OF FIRST
    // ENCOUNTER (keyframes ascending, each keyframe's getKeypoints3d() order), and that order decides the matcher's ties.
    void assembleLoopLocalMap(const Frame &newkf, const Frame &lckf, std::vector<std::pair<int, int>> &vkplmids, LoopLocalMap &in) const;
    // :502-583 for B pairs: assembleLoopLocalMap on each, then ONE ov2_loop_match_to_map_batch call (one synchronisation) for
    // the pairs that have keypoints and candidates, whatever B is; the new pairs of each job are appended to its vkplmids in
    // ascending keypoint-lmid order (the reference's std::map).  The keypoints go to the kernel in the order of the new
    // keyframe's grid, the candidates in vcands' order.  Every new keyframe needs a grid of one cell size and the map's one left
    // camera (else OV2_ERR_INVALID); a keyframe that is not in the map is OV2_ERR_INVALID.
    ov2_status trackLoopLocalMaps(std::vector<LoopTrackJob> &jobs, float maxdist, float ratio);
    // :502-583 as written, one pair: trackLoopLocalMaps with B = 1
    ov2_status trackLoopLocalMap(const Frame &newkf, const Frame &lckf, const SE3 &Twc, float maxdist, float ratio,
                                 std::vector<std::pair<int, int>> &vkplmids);
    LoopTrackStats last_track_;
    LoopTrackJob last_track_job_;   // the counts of the last trackLoopLocalMap call (its list is not kept)
    // :834-897 as written -> MultiViewGeometry::ceresPnP (10 iterations, robust_mono_th_, robust, no L2 re-solve): pairs whose
    // map point is gone or whose keypoint the frame does not hold stay out, the solver's outliers are mapped back through
    // vgoodkpidx and APPENDED to voutlier_idx; fewer than 3 correspondences: false
    bool computePnP(const Frame &frame, const std::vector<std::pair<int, int>> &vkplmids, SE3 &Twc, std::vector<int> &voutlier_idx);
    // :765-831 as written: pairs whose map point is gone are ERASED from vkplmids (vbadidx), fewer than 4 -> false, RANSAC with
    // 10 * nransac_iter_ draws (ov2_p3p_ransac_batch, use_lmeds = 0), and do_optimize = true through refineP3P
    bool p3pRansac(const Frame &newkf, std::vector<std::pair<int, int>> &vkplmids, std::vector<int> &voutliers_idx, SE3 &Twc,
                   uint64_t seed, ov2_status *st = nullptr, int *status = nullptr, int *info = nullptr);
    // What stands for OpenGV's optimizeModelCoefficients (do_optimize) after a successful RANSAC, for B poses in one
    // ov2_pnp_solve_batch call: a motion-only solve on each pair's RANSAC inliers with bz > 0, pixels (fx bx / bz, fy by / bz),
    // K = (fx, fy, 0, 0) (no principal point is known here and it cancels), no scales, 10 iterations, chi2 5.9915, robust, no
    // L2 re-solve (computePnP's settings).  Its outlier flags are ignored; a pose whose solve returns success = 0 stays RANSAC's.
    // n / bvs / wpts / outlier: the pairs' correspondences one after the other; Twc: B x 7, in / out
    static ov2_status refineP3P(ov2_ctx *ctx, int B, const int *n, const double *bvs, const double *wpts, const uint8_t *outlier,
                                const double *K, double *Twc);
    // :238-300 as written, one pair: p3pRansac, removeOutliers, trackLoopLocalMap, computePnP, one call and one synchronisation
    // per stage.  vkplmids: the list the 2D-2D half passed on
    ov2_status verifyLoopCandidate(int newkfid, int lckfid, const std::vector<std::pair<int, int>> &vkplmids, uint64_t seed,
                                   LoopVerifyResult &r);
    // the same for B pairs: ONE ov2_p3p_ransac_batch call, ONE refinement call, ONE ov2_loop_match_to_map_batch call and ONE
    // ov2_pnp_solve_batch call whatever B is, each for the pairs that reach that stage; the counts are kept in last_
    ov2_status verifyLoopCandidates(const std::vector<std::pair<int, int>> &pairs, const std::vector<std::vector<std::pair<int, int>>> &lists,
                                    const std::vector<uint64_t> &seeds, std::vector<LoopVerifyResult> &out);
    // matchLoopCandidates, then verifyLoopCandidates for the pairs that ended LC_PASSED (against the candidate it used)
    ov2_status processLoopCandidates(const std::vector<std::pair<int, int>> &pairs, const std::vector<uint64_t> &seeds,
                                     std::vector<LoopPairResult> &matched, std::vector<LoopVerifyResult> &verified);
    // :380-424, the part of knnMatching in front of the matcher: identity pairs, query and train sets (no GPU)
    void assembleKnn(const Frame &newkf, const Frame &lckf, LoopKnnInputs &in) const;
    // :430-449: maxdist, the ratio test in double, (kpid, lmid) of the accepted matches appended to vkplmids; idx / dist:
    // n_query x 2 as ov2_knn2_hamming_batch writes them
    static void acceptMatches(const LoopKnnInputs &in, const int32_t *idx, const int32_t *dist, std::vector<std::pair<int, int>> &vkplmids);
    static bool acceptMatch(int d0, int d1);   // :434-442, d1 < 0: fewer than 2 neighbours
    // :378-459, ov2_knn2_hamming_batch with B = 1
    ov2_status knnMatching(const Frame &newkf, const Frame &lckf, std::vector<std::pair<int, int>> &vkplmids);
    // :462-499 -> MultiViewGeometry::compute5ptEssentialMatrix (10 nransac_iter_ iterations, fransac_err_, no optimisation);
    // seed replaces the reference's bdo_random clock seed
    bool epipolarFiltering(const Frame &newkf, const Frame &lckf, std::vector<std::pair<int, int>> &vkplmids,
                           std::vector<int> &voutliers_idx, uint64_t seed, ov2_status *st = nullptr);
    // :899-928, as written: voutliers_idx must ascend, and once its last entry is met j wraps to 0 with entry 0 set to -1
    static void removeOutliers(std::vector<std::pair<int, int>> &vkplmids, std::vector<int> &voutliers_idx);
    // :184-236 as written, one candidate: knnMatching, epipolarFiltering, removeOutliers one after the other (a synchronisation
    // each).  Fills the same fields as matchLoopCandidates except epi_info, R and t, which the reference's call does not return.
    ov2_status processLoopCandidate(int newkfid, int lckfid, uint64_t seed, LoopPairResult &r);
    // :184-236 for B pairs (newkfid, candidate kfid) of this map: one ov2_knn2_hamming_batch call for all pairs that reach the
    // matcher, one ov2_epipolar_filter_batch call for all that reach the filter (two synchronisations whatever B is); B = 1
    // is the reference's call.  seeds: one sampler seed per pair.  A new keyframe that is not in the map is OV2_ERR_INVALID.
    ov2_status matchLoopCandidates(const std::vector<std::pair<int, int>> &pairs, const std::vector<uint64_t> &seeds,
                                   std::vector<LoopPairResult> &out);
    LoopStats last_;
    // :302-372, statement by statement: the >= 30 gate; inikfid = the smallest key of the loop keyframe's covisibility map
    // (DEPARTURE: an empty map is undefined behaviour in the reference, here it stands for the keyframe's own id);
    // lc_pose_err; localPoseGraph; on success mergeMapPoints for every pair with prev != new in list order,
    // structureOnlyBA(vmergedlmids) and, if lc_pose_err >= 0.02, looseBA(smallest key of inikf's covisibility map, newkfid,
    // true).  A keyframe that is not in the map is OV2_ERR_INVALID.  closeLoop is closeLoops with one job.
    ov2_status closeLoop(int newkfid, int lckfid, const SE3 &Twc, const std::vector<std::pair<int, int>> &vkplmids, LoopCloseResult &r);
    // the same for B closers with distinct maps on one context: every job's graph is assembled, ONE
    // ov2_pose_graph_solve_batch call solves the graphs of the jobs that pass the gate and have a chain (a graph that the
    // degenerate test then refuses has been solved: it counts as offered), then apply / merge / structureOnlyBA / looseBA
    // per job -- the two BA calls stay one library call per job.  A job's outcome equals closeLoop on it.
    static ov2_status closeLoops(std::vector<LoopCloseJob> &jobs);
    LoopCloseStats last_close_;
    LoopCloseResult last_closed_;   // `closed` of the last newKeyframe result handed out through the C hooks
    bool close_loops_ = false;
    ov2_ctx *ctx_;
    std::shared_ptr<SlamParams> pslamstate_;
    std::shared_ptr<MapManager> pmap_;

private:
    // :97-109: the descriptors of the keyframe's map points (and, with px, the pixels of those keypoints); false: no such keyframe
    bool mapPointDescs(int kfid, std::vector<uint8_t> &descs, std::vector<Point2f> *px, int *nbkps) const;
    // :187-195 and :167 behind a detector result
    ov2_status afterDetector(int kfid, uint64_t seed, LoopNewKeyframeResult &r, bool close_now = true);
};

}  // namespace ov2
