// ov2_host_capi.cpp -- flat C hooks around the C++ host mirror so that pytest can build a Frame/MapPoint graph,
// run Optimizer::setupLocalBA (CPU only) or the whole Estimator::applyLocalBA (GPU) and read the map back.
// Test/bring-up surface only; a real integration uses the C++ classes of ov2_host.hpp directly.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

#include "ov2_host.hpp"
#include "ov2_lcd.hpp"
#include "ov2_slam.hpp"

using namespace ov2;

namespace {
struct HostMap {
    std::shared_ptr<SlamParams> st = std::make_shared<SlamParams>();
    std::shared_ptr<MapManager> map = std::make_shared<MapManager>();
    std::shared_ptr<CameraCalibration> cl = std::make_shared<CameraCalibration>(), cr = std::make_shared<CameraCalibration>();
    LocalBAProblem pb;
    bool bp3preq = false;    // VisualFrontEnd::bp3preq_, carried from one ov2h_compute_pose call to the next
    P3pStats last_p3p;       // the P3P branch of the last ov2h_compute_pose
    EpiStats last_epi;       // the last ov2h_epipolar_filtering / ov2h_check_ready_for_init
};
}  // namespace

extern "C" {

void *ov2h_map_create(int stereo, int inv_depth, const double *Kl, const double *Kr, const double *T_lr7, int w, int h,
                      int nmin_covscore)
{
    HostMap *m = new HostMap();
    m->st->stereo_ = stereo != 0; m->st->mono_ = !stereo; m->st->buse_inv_depth_ = inv_depth != 0;
    m->st->nmin_covscore_ = nmin_covscore;
    m->cl->fx_ = Kl[0]; m->cl->fy_ = Kl[1]; m->cl->cx_ = Kl[2]; m->cl->cy_ = Kl[3]; m->cl->img_w_ = w; m->cl->img_h_ = h;
    m->cr->fx_ = Kr[0]; m->cr->fy_ = Kr[1]; m->cr->cx_ = Kr[2]; m->cr->cy_ = Kr[3]; m->cr->img_w_ = w; m->cr->img_h_ = h;
    for (int i = 0; i < 7; ++i) m->cr->Tc0ci_.v[i] = T_lr7[i];
    return m;
}

void ov2h_map_destroy(void *p) { delete (HostMap *)p; }

int ov2h_map_add_keyframe(void *p, int kfid, const double *Twc7)
{
    HostMap *m = (HostMap *)p;
    auto f = std::make_shared<Frame>();
    f->id_ = kfid; f->kfid_ = kfid;
    f->pcalib_leftcam_ = m->cl; f->pcalib_rightcam_ = m->cr;
    SE3 T;
    for (int i = 0; i < 7; ++i) T.v[i] = Twc7[i];
    f->setTwc(T);
    m->map->map_pkfs_[kfid] = f;
    return 0;
}

int ov2h_map_add_landmark(void *p, int lmid, const double *xyz, int anchor_kfid)
{
    HostMap *m = (HostMap *)p;
    auto lm = std::make_shared<MapPoint>(lmid, anchor_kfid, true);
    lm->set_kfids_.clear();
    lm->setPoint(Vec3{xyz[0], xyz[1], xyz[2]});
    m->map->map_plms_[lmid] = lm;
    return 0;
}

int ov2h_map_add_obs(void *p, int kfid, int lmid, float ux, float uy, int is_stereo, float rux, float ruy)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    auto lm = m->map->getMapPoint(lmid);
    if (!f || !lm) return -1;
    Keypoint kp;
    kp.lmid_ = lmid; kp.px_ = {ux, uy}; kp.unpx_ = {ux, uy}; kp.is3d_ = true;
    kp.is_stereo_ = is_stereo != 0; kp.rpx_ = {rux, ruy}; kp.runpx_ = {rux, ruy};
    f->addKeypoint(kp);
    lm->addKfObs(kfid);
    return 0;
}

// a keypoint of keyframe kfid that is 2D or 3D (is3d); the map point is created on first use (2D ones carry no position)
int ov2h_map_add_kp(void *p, int kfid, int lmid, float ux, float uy, int is3d, const double *xyz)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    auto lm = m->map->getMapPoint(lmid);
    if (!lm) {
        lm = std::make_shared<MapPoint>(lmid, kfid, true);
        if (is3d && xyz) lm->setPoint(Vec3{xyz[0], xyz[1], xyz[2]});
        m->map->map_plms_[lmid] = lm;
    }
    Keypoint kp;
    kp.lmid_ = lmid;
    f->computeKeypoint(Point2f{ux, uy}, kp);
    kp.is3d_ = is3d != 0;
    f->addKeypoint(kp);
    lm->addKfObs(kfid);
    return 0;
}

int ov2h_frame_init_grid(void *p, int kfid, int ncellsize)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    f->initGrid((size_t)ncellsize);
    return 0;
}

// drops a map point but leaves the keypoints that reference it (the "plm == nullptr" branch of stereoMatching, :414)
int ov2h_map_forget_landmark(void *p, int lmid) { ((HostMap *)p)->map->map_plms_.erase(lmid); return 0; }

// ---- a host map of N keyframes with chosen 2D / 3D keypoints (tests of Mapper::triangulateTemporal) ----
// n keypoints of keyframe kfid; a map point is created on first use, 3D at xyz[3 i ..] when lm3d[i] is set, and the keypoint
// carries Keypoint::is3d_ = kp3d[i]
int ov2h_map_add_kps(void *p, int kfid, int n, const int *lmid, const float *uv, const uint8_t *kp3d, const uint8_t *lm3d, const double *xyz)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    for (int i = 0; i < n; ++i) {
        auto lm = m->map->getMapPoint(lmid[i]);
        if (!lm) {
            lm = std::make_shared<MapPoint>(lmid[i], kfid, true);
            if (lm3d[i]) lm->setPoint(Vec3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
            m->map->map_plms_[lmid[i]] = lm;
        }
        Keypoint kp;
        kp.lmid_ = lmid[i];
        f->computeKeypoint(Point2f{uv[2 * i], uv[2 * i + 1]}, kp);
        kp.is3d_ = kp3d[i] != 0;
        f->addKeypoint(kp);
        lm->addKfObs(kfid);
    }
    return 0;
}

// drops a keyframe but leaves it in the observer sets of its map points (the "pkf == nullptr" branch, src/mapper.cpp:271)
int ov2h_map_forget_keyframe(void *p, int kfid) { ((HostMap *)p)->map->map_pkfs_.erase(kfid); return 0; }

// drops a keypoint of keyframe kfid but leaves the keyframe among the observers of its map point (src/mapper.cpp:292-295)
int ov2h_map_forget_kp(void *p, int kfid, int lmid)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    f->removeKeypointById(lmid);
    return 0;
}

// Mapper::triangulateTemporal on keyframe kfid.  lmid / branch (capacity cap): the keypoints offered, ids ascending, and the
// ov2::TemporalBranch each one took; stats[4]: 2D keypoints offered, candidates, good, observations removed.  Returns the
// number of keypoints offered, or -1 - status
int ov2h_triangulate_temporal(void *p, void *ctx, int kfid, float max_reproj_err, int cap, int *lmid, int *branch, double *stats)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1 - (int)OV2_ERR_INVALID;
    m->st->fmax_reproj_err_ = max_reproj_err;
    TemporalStats ts;
    const ov2_status s = SlamManager::triangulateTemporal((ov2_ctx *)ctx, *m->map, *m->st, *f, ts);
    if (s != OV2_OK) return -1 - (int)s;
    for (int i = 0; i < ts.n_kps && i < cap; ++i) { lmid[i] = ts.lmid[i]; branch[i] = ts.branch[i]; }
    if (stats) { stats[0] = ts.n_kps; stats[1] = ts.n_candidates; stats[2] = ts.n_good; stats[3] = ts.n_removed; }
    return ts.n_kps;
}

// ---- Mapper::triangulateStereo on a host map ----
// Frame::updateKeypointStereo(lmid[i], rxy[i]) on keyframe kfid for n keypoints (raw right pixels; the right camera of the map
// undistorts them); a keyframe the device mirror already holds gets the rows with the next flush
int ov2h_map_set_kp_stereo(void *p, int kfid, int n, const int *lmid, const float *rxy)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f || n < 0) return f ? -2 : -1;
    for (int i = 0; i < n; ++i) {
        if (!f->isObservingKp(lmid[i])) continue;
        f->updateKeypointStereo(lmid[i], Point2f{rxy[2 * i], rxy[2 * i + 1]});
        m->map->touchStereoOn(kfid, lmid[i]);
    }
    return 0;
}

// the right camera of the map: intrinsics, extrinsic (Tc0ci_, t then qx qy qz qw) and SlamParams::bdo_stereo_rect_
int ov2h_map_set_right_cam(void *p, const double *Kr, const double *T_lr7, int rectified)
{
    HostMap *m = (HostMap *)p;
    m->cr->fx_ = Kr[0]; m->cr->fy_ = Kr[1]; m->cr->cx_ = Kr[2]; m->cr->cy_ = Kr[3];
    for (int i = 0; i < 7; ++i) m->cr->Tc0ci_.v[i] = T_lr7[i];
    m->st->bdo_stereo_rect_ = rectified != 0;
    return 0;
}

// Mapper::triangulateStereo on keyframe kfid.  lmid / verdict (capacity cap): the keypoints offered, ids ascending, and the
// OV2_TRI_* verdict of each; stats[3]: stereo 2D keypoints offered, good, demoted.  Returns the number of keypoints offered,
// or -1 - status
int ov2h_triangulate_stereo(void *p, void *ctx, int kfid, float max_reproj_err, int cap, int *lmid, int *verdict, double *stats)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1 - (int)OV2_ERR_INVALID;
    m->st->fmax_reproj_err_ = max_reproj_err;
    StereoTriStats ts;
    const ov2_status s = SlamManager::triangulateStereo((ov2_ctx *)ctx, *m->map, *m->st, *f, ts);
    if (s != OV2_OK) return -1 - (int)s;
    for (int i = 0; i < ts.n_kps && i < cap; ++i) { lmid[i] = ts.lmid[i]; verdict[i] = ts.verdict[i]; }
    if (stats) { stats[0] = ts.n_kps; stats[1] = ts.n_good; stats[2] = ts.n_demoted; }
    return ts.n_kps;
}

// Estimator::mapFiltering on a host map with keyframe newkf as the new keyframe (no GPU context needed; with a device mirror
// attached the removals reach it through MapManager::removeKeyframe).  removed_kfid (capacity cap): removed ids in order;
// stats[4]: ran, candidates examined, removed by the nb3dkps_ rule, landmarks whose is3d_ isBad() cleared.  Returns the number
// of keyframes removed, or -1 - status
int ov2h_map_filtering(void *p, int newkf, int nmin_covscore, float ratio, int cap, int *removed_kfid, double *stats)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f) return -1 - (int)OV2_ERR_INVALID;
    m->st->nmin_covscore_ = nmin_covscore; m->st->fkf_filtering_ratio_ = ratio;
    Estimator est(m->st, m->map, nullptr);
    est.pnewkf_ = f;
    const ov2_status s = est.mapFiltering();
    if (s != OV2_OK) return -1 - (int)s;
    const FilterStats &fs = est.last_filter_;
    for (size_t i = 0; i < fs.removed.size() && (int)i < cap; ++i) removed_kfid[i] = fs.removed[i];
    if (stats) { stats[0] = fs.ran; stats[1] = fs.n_candidates; stats[2] = fs.n_few3d; stats[3] = (double)fs.unset3d.size(); }
    return (int)fs.removed.size();
}

// ---- loop-candidate matching (ov2::LoopCloser, the 2D-2D half of processLoopCandidate) ----
// MapPoint::addDesc(kfid, desc) on landmark lmid: the descriptor keyframe kfid holds of it (the first one becomes desc_)
int ov2h_map_add_desc(void *p, int lmid, int kfid, const uint8_t *desc32)
{
    auto lm = ((HostMap *)p)->map->getMapPoint(lmid);
    if (!lm) return -1;
    Desc d;
    std::copy(desc32, desc32 + 32, d.begin());
    lm->addDesc(kfid, d);
    ((HostMap *)p)->map->touchDesc(lmid);
    return 0;
}

// Frame::map_covkfs_[other] = score on keyframe kfid (the covisibility gate of processLoopCandidate reads it)
int ov2h_map_set_covscore(void *p, int kfid, int other, int score)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    f->map_covkfs_[other] = score;
    return 0;
}

// ---- the local map of a keyframe (MapManager::updateFrameCovisibility, the set assembly of Mapper::matchingToLocalMap); no
// hook below needs a GPU context.  Returns are 0 (or the value named) or a negative number: -1 = the keyframe is not in the map
// MapManager::updateFrameCovisibility on keyframe kfid: Frame::map_covkfs_ and Frame::set_local_mapids_ of the keyframe
int ov2h_update_frame_covisibility(void *p, int kfid)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    m->map->updateFrameCovisibility(*f);
    return 0;
}

// SlamManager::extendLocalMap on keyframe kfid: 1 = the extension branch was taken, 0 = it was not
int ov2h_extend_local_map(void *p, int kfid, int nmax_local)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f || nmax_local < 0) return f ? -2 : -1;
    return SlamManager::extendLocalMap(*m->map, *f, (size_t)nmax_local) ? 1 : 0;
}

// Frame::set_local_mapids_ of keyframe kfid in its own iteration order: *n = its size, the first min(cap, *n) ids in out
int ov2h_frame_local_ids(void *p, int kfid, int cap, int *out, int *n)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    int i = 0;
    for (int l : f->set_local_mapids_) { if (i < cap) out[i] = l; ++i; }
    *n = i;
    return 0;
}

// Frame::set_local_mapids_ of keyframe kfid becomes the n ids (duplicates collapse, as in any set)
int ov2h_frame_set_local_ids(void *p, int kfid, int n, const int *ids)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f || n < 0) return f ? -2 : -1;
    f->set_local_mapids_.clear();
    f->set_local_mapids_.insert(ids, ids + n);
    return 0;
}

// Frame::map_covkfs_ of keyframe kfid, ascending kfid: *n = its size, the first min(cap, *n) entries in kfids / scores
int ov2h_frame_cov_map(void *p, int kfid, int cap, int *kfids, int *scores, int *n)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    int i = 0;
    for (const auto &c : f->map_covkfs_) { if (i < cap) { kfids[i] = c.first; scores[i] = c.second; } ++i; }
    *n = i;
    return 0;
}

// what LoopCloser::knnMatching assembles for the pair (newkf, lckf) in front of the matcher, no GPU context needed: query
// lmids, train lmids and identity pairs (one lmid each) in the mirror's own iteration order, capacity cap each; n[3] = their
// counts.  query_desc / train_desc (cap x 32, may be NULL): the rows the matcher would receive
int ov2h_loop_assemble(void *p, int newkf, int lckf, int cap, int *n, int *query_lmid, int *train_lmid, int *identity_lmid,
                       uint8_t *query_desc, uint8_t *train_desc)
{
    HostMap *m = (HostMap *)p;
    auto a = m->map->getKeyframe(newkf), b = m->map->getKeyframe(lckf);
    if (!a || !b) return (int)OV2_ERR_INVALID;
    LoopCloser lc(nullptr, m->st, m->map);
    LoopKnnInputs in;
    lc.assembleKnn(*a, *b, in);
    n[0] = (int)in.vkpids.size(); n[1] = (int)in.vlmids.size(); n[2] = (int)in.vkplmids.size();
    if (n[0] > cap || n[1] > cap || n[2] > cap) return (int)OV2_ERR_INVALID;
    std::copy(in.vkpids.begin(), in.vkpids.end(), query_lmid);
    std::copy(in.vlmids.begin(), in.vlmids.end(), train_lmid);
    for (int i = 0; i < n[2]; ++i) identity_lmid[i] = in.vkplmids[i].first;
    if (query_desc) std::copy(in.query.begin(), in.query.end(), query_desc);
    if (train_desc) std::copy(in.train.begin(), in.train.end(), train_desc);
    return 0;
}

// what LoopCloser::trackLoopLocalMap assembles for the pair (newkf, lckf) in front of its matcher (assembleLoopLocalMap), no
// GPU context needed.  pairs_in (n_in x 2): the incoming vkplmids.  pairs_out (cap x 2): vkplmids with the identity pairs
// appended; matched / local / cands (cap each): vmatchedkpids, the local set and the candidates offered to the matcher, the
// last two in the mirror's order of first encounter.  n[4] = their counts; OV2_ERR_INVALID when one exceeds cap
int ov2h_loop_local_map(void *p, int newkf, int lckf, int n_in, const int *pairs_in, int cap, int *n, int *pairs_out, int *matched,
                        int *local, int *cands)
{
    HostMap *m = (HostMap *)p;
    auto a = m->map->getKeyframe(newkf), b = m->map->getKeyframe(lckf);
    if (!a || !b || n_in < 0) return (int)OV2_ERR_INVALID;
    LoopCloser lc(nullptr, m->st, m->map);
    std::vector<std::pair<int, int>> v((size_t)n_in);
    for (int i = 0; i < n_in; ++i) v[i] = {pairs_in[2 * i], pairs_in[2 * i + 1]};
    LoopLocalMap in;
    lc.assembleLoopLocalMap(*a, *b, v, in);
    n[0] = (int)v.size(); n[1] = (int)in.vmatchedkpids.size(); n[2] = (int)in.vlocal.size(); n[3] = (int)in.vcands.size();
    if (n[0] > cap || n[1] > cap || n[2] > cap || n[3] > cap) return (int)OV2_ERR_INVALID;
    for (size_t i = 0; i < v.size(); ++i) { pairs_out[2 * i] = v[i].first; pairs_out[2 * i + 1] = v[i].second; }
    std::copy(in.vmatchedkpids.begin(), in.vmatchedkpids.end(), matched);
    std::copy(in.vlocal.begin(), in.vlocal.end(), local);
    std::copy(in.vcands.begin(), in.vcands.end(), cands);
    return in.n_identity;
}

// LoopCloser::trackLoopLocalMaps on B jobs (newkf[b], lckf[b], Twc (B x 7), the incoming pair lists one after the other:
// n_in[b] pairs each in pairs_in).  pairs_out (cap x 2): the lists after tracking, job after job, n_out[b] pairs each; counts
// (B x 3): identity pairs appended, candidates offered, matches appended; stats[3]: jobs, offered to the matcher, launches.
// Returns 0 or a negative ov2_status (OV2_ERR_INVALID also when cap is too small)
int ov2h_loop_track(void *p, void *ctx, int B, const int *newkf, const int *lckf, const double *Twc7, float maxdist, float ratio,
                    const int *n_in, const int *pairs_in, int cap, int *n_out, int *pairs_out, int *counts, int *stats)
{
    HostMap *m = (HostMap *)p;
    if (B < 0) return (int)OV2_ERR_INVALID;
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<LoopTrackJob> jobs((size_t)B);
    size_t o = 0;
    for (int b = 0; b < B; ++b) {
        jobs[b].newkfid = newkf[b]; jobs[b].lckfid = lckf[b];
        for (int i = 0; i < 7; ++i) jobs[b].Twc.v[i] = Twc7[7 * b + i];
        if (n_in[b] < 0) return (int)OV2_ERR_INVALID;
        for (int i = 0; i < n_in[b]; ++i, ++o) jobs[b].vkplmids.push_back({pairs_in[2 * o], pairs_in[2 * o + 1]});
    }
    const ov2_status s = lc.trackLoopLocalMaps(jobs, maxdist, ratio);
    if (s != OV2_OK) return (int)s;
    o = 0;
    for (int b = 0; b < B; ++b) {
        const LoopTrackJob &j = jobs[b];
        if (o + j.vkplmids.size() > (size_t)cap) return (int)OV2_ERR_INVALID;
        n_out[b] = (int)j.vkplmids.size();
        counts[3 * b] = j.n_identity; counts[3 * b + 1] = j.n_offered; counts[3 * b + 2] = j.n_matched;
        for (const auto &q : j.vkplmids) { pairs_out[2 * o] = q.first; pairs_out[2 * o + 1] = q.second; ++o; }
    }
    stats[0] = lc.last_track_.pairs; stats[1] = lc.last_track_.match_pairs; stats[2] = lc.last_track_.match_calls;
    return 0;
}

// LoopCloser::computePnP (:834-897) on keyframe kfid with n pairs (kpid, lmid) and the start pose Twc7 (updated in place);
// outidx (cap): the n_out_in indices it is given followed by those it appends, *n_out their count.  Returns its bool (0 / 1)
// or a negative ov2_status
int ov2h_loop_compute_pnp(void *p, void *ctx, int kfid, int n, const int *pairs, double *Twc7, int n_out_in, int cap, int *outidx, int *n_out)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f || n < 0 || n_out_in < 0 || n_out_in > cap) return (int)OV2_ERR_INVALID;
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> v((size_t)n);
    for (int i = 0; i < n; ++i) v[i] = {pairs[2 * i], pairs[2 * i + 1]};
    std::vector<int> out(outidx, outidx + n_out_in);
    SE3 T;
    for (int i = 0; i < 7; ++i) T.v[i] = Twc7[i];
    const bool ok = lc.computePnP(*f, v, T, out);
    if (out.size() > (size_t)cap) return (int)OV2_ERR_INVALID;
    for (int i = 0; i < 7; ++i) Twc7[i] = T.v[i];
    std::copy(out.begin(), out.end(), outidx);
    *n_out = (int)out.size();
    return ok ? 1 : 0;
}

// One LoopVerifyResult as flat arrays.  ints[13]: branch (ov2::LoopVerifyBranch), P3P status (-1 = not run), its info[4], pairs after
// P3P, after tracking, at the end, identity pairs appended, candidates offered, matches found, computePnP outliers; dbl[15]: Twc after
// P3P + refinement, final Twc, lc_pose_err; lists: the three pair lists (2 ints per pair) and the outlier indices, one after the
// other, appended at *used (capacity cap ints).  false = cap too small
static bool pack_verify(const LoopVerifyResult &r, int *ints, double *dbl, int cap, int *lists, size_t *used)
{
    ints[0] = r.branch; ints[1] = r.p3p_status; std::copy(r.p3p_info, r.p3p_info + 4, ints + 2);
    ints[6] = (int)r.vkplmids_p3p.size(); ints[7] = (int)r.vkplmids_track.size(); ints[8] = (int)r.vkplmids.size();
    ints[9] = r.n_identity; ints[10] = r.n_offered; ints[11] = r.n_matched; ints[12] = (int)r.pnp_outliers.size();
    std::copy(r.Twc_p3p.v.begin(), r.Twc_p3p.v.end(), dbl); std::copy(r.Twc.v.begin(), r.Twc.v.end(), dbl + 7); dbl[14] = r.lc_pose_err;
    const size_t need = 2 * (r.vkplmids_p3p.size() + r.vkplmids_track.size() + r.vkplmids.size()) + r.pnp_outliers.size();
    if (*used + need > (size_t)cap) return false;
    int *o = lists + *used;
    for (const auto *v : {&r.vkplmids_p3p, &r.vkplmids_track, &r.vkplmids})
        for (const auto &q : *v) { *o++ = q.first; *o++ = q.second; }
    for (int i : r.pnp_outliers) *o++ = i;
    *used += need;
    return true;
}

static void loop_params(HostMap *m, int nransac_iter, float fransac_err) { m->st->nransac_iter_ = nransac_iter; m->st->fransac_err_ = fransac_err; }

// LoopCloser::verifyLoopCandidates on B pairs (newkf[b], lckf[b]) with their incoming lists one after the other (n_in[b] pairs
// each in pairs_in) and one sampler seed each.  ints (B x 13), dbl (B x 15), lists (cap ints): pack_verify, pair after pair.
// stats[8]: pairs that reached P3P, the refinement, the matcher, computePnP, and the library calls of each stage.
// Returns 0 or a negative ov2_status (OV2_ERR_INVALID also when cap is too small)
int ov2h_loop_verify(void *p, void *ctx, int B, const int *newkf, const int *lckf, const int *n_in, const int *pairs_in,
                     const unsigned long long *seeds, int nransac_iter, float fransac_err, int cap, int *ints, double *dbl, int *lists,
                     int *stats)
{
    HostMap *m = (HostMap *)p;
    if (B < 0) return (int)OV2_ERR_INVALID;
    loop_params(m, nransac_iter, fransac_err);
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> pairs((size_t)B);
    std::vector<std::vector<std::pair<int, int>>> vl((size_t)B);
    std::vector<uint64_t> sd((size_t)B);
    size_t o = 0;
    for (int b = 0; b < B; ++b) {
        pairs[b] = {newkf[b], lckf[b]}; sd[b] = (uint64_t)seeds[b];
        if (n_in[b] < 0) return (int)OV2_ERR_INVALID;
        for (int i = 0; i < n_in[b]; ++i, ++o) vl[b].push_back({pairs_in[2 * o], pairs_in[2 * o + 1]});
    }
    std::vector<LoopVerifyResult> out;
    const ov2_status s = lc.verifyLoopCandidates(pairs, vl, sd, out);
    if (s != OV2_OK) return (int)s;
    size_t used = 0;
    for (int b = 0; b < B; ++b)
        if (!pack_verify(out[b], ints + 13 * b, dbl + 15 * b, cap, lists, &used)) return (int)OV2_ERR_INVALID;
    const LoopStats &L = lc.last_;
    const int st[8] = {L.p3p_pairs, L.refine_pairs, L.track_pairs, L.pnp_pairs, L.p3p_calls, L.refine_calls, L.track_calls, L.pnp_calls};
    std::copy(st, st + 8, stats);
    return 0;
}

// LoopCloser::verifyLoopCandidate, the reference-shaped call on one pair (a call and a synchronisation per stage); outputs as
// one row of ov2h_loop_verify
int ov2h_loop_verify_candidate(void *p, void *ctx, int newkf, int lckf, int n_in, const int *pairs_in, unsigned long long seed,
                               int nransac_iter, float fransac_err, int cap, int *ints, double *dbl, int *lists)
{
    HostMap *m = (HostMap *)p;
    if (n_in < 0) return (int)OV2_ERR_INVALID;
    loop_params(m, nransac_iter, fransac_err);
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> v((size_t)n_in);
    for (int i = 0; i < n_in; ++i) v[i] = {pairs_in[2 * i], pairs_in[2 * i + 1]};
    LoopVerifyResult r;
    const ov2_status s = lc.verifyLoopCandidate(newkf, lckf, v, (uint64_t)seed, r);
    if (s != OV2_OK) return (int)s;
    size_t used = 0;
    return pack_verify(r, ints, dbl, cap, lists, &used) ? 0 : (int)OV2_ERR_INVALID;
}

// one LoopCloseResult as flat rows: ints[9] = branch, inikfid, looseBA's start id, status of the pose-graph solve, of
// structureOnlyBA, of looseBA (ov2::LCL_NOT_CALLED = 1 where the call was not made), merged lmids, termination and log
// entries of the pose graph; dbl[3] = lc_pose_err, initial and final cost of the pose graph; merged: the lmids (room for cap)
static bool pack_close(const LoopCloseResult &r, int *ints, double *dbl, int cap, int *merged)
{
    const int v[9] = {r.branch, r.inikfid, r.loose_start, r.pg_status, r.sba_status, r.loose_status, (int)r.vmergedlmids.size(),
                      r.pg.termination, r.pg.n_log};
    std::copy(v, v + 9, ints);
    dbl[0] = r.lc_pose_err; dbl[1] = r.pg.initial_cost; dbl[2] = r.pg.final_cost;
    if ((int)r.vmergedlmids.size() > cap) return false;
    std::copy(r.vmergedlmids.begin(), r.vmergedlmids.end(), merged);
    return true;
}

// LoopCloser::closeLoop on one accepted loop; stats[3] = last_close_ (jobs, graphs offered, solve calls).  0 or a negative ov2_status
int ov2h_loop_close(void *p, void *ctx, int newkf, int lckf, const double *Twc7, int n, const int *pairs, int cap, int *ints, double *dbl,
                    int *merged, int *stats)
{
    HostMap *m = (HostMap *)p;
    if (n < 0) return (int)OV2_ERR_INVALID;
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> v((size_t)n);
    for (int i = 0; i < n; ++i) v[i] = {pairs[2 * i], pairs[2 * i + 1]};
    SE3 T;
    for (int k = 0; k < 7; ++k) T.v[k] = Twc7[k];
    LoopCloseResult r;
    const ov2_status s = lc.closeLoop(newkf, lckf, T, v, r);
    stats[0] = lc.last_close_.jobs; stats[1] = lc.last_close_.graphs; stats[2] = lc.last_close_.solve_calls;
    if (s != OV2_OK) return (int)s;
    return pack_close(r, ints, dbl, cap, merged) ? 0 : (int)OV2_ERR_INVALID;
}

// LoopCloser::closeLoops on B maps (one accepted loop each): rows of ov2h_loop_close per map (ints B x 9, dbl B x 3, merged
// B x cap), n_pairs[b] pairs of map b one after the other in `pairs`
int ov2h_loop_close_batch(int B, void *const *maps, void *ctx, const int *newkf, const int *lckf, const double *Twc7, const int *n_pairs,
                          const int *pairs, int cap, int *ints, double *dbl, int *merged, int *stats)
{
    if (B < 0) return (int)OV2_ERR_INVALID;
    std::vector<std::unique_ptr<LoopCloser>> closers;
    std::vector<LoopCloseJob> jobs((size_t)B);
    size_t o = 0;
    for (int b = 0; b < B; ++b) {
        HostMap *m = (HostMap *)maps[b];
        if (!m || n_pairs[b] < 0) return (int)OV2_ERR_INVALID;
        closers.emplace_back(new LoopCloser((ov2_ctx *)ctx, m->st, m->map));
        LoopCloseJob &J = jobs[b];
        J.closer = closers.back().get(); J.newkfid = newkf[b]; J.lckfid = lckf[b];
        for (int k = 0; k < 7; ++k) J.Twc.v[k] = Twc7[7 * (size_t)b + k];
        for (int i = 0; i < n_pairs[b]; ++i, ++o) J.vkplmids.push_back({pairs[2 * o], pairs[2 * o + 1]});
    }
    const ov2_status s = LoopCloser::closeLoops(jobs);
    stats[0] = stats[1] = stats[2] = 0;
    if (B) { const LoopCloseStats &L = closers[0]->last_close_; stats[0] = L.jobs; stats[1] = L.graphs; stats[2] = L.solve_calls; }
    if (s != OV2_OK) return (int)s;
    for (int b = 0; b < B; ++b)
        if (!pack_close(jobs[b].r, ints + 9 * (size_t)b, dbl + 3 * (size_t)b, cap, merged + (size_t)cap * b)) return (int)OV2_ERR_INVALID;
    return 0;
}

// MapManager::mergeMapPoints(prevlmid, newlmid), so that a test can walk the chain step by step
int ov2h_map_merge_points(void *p, int prevlmid, int newlmid)
{
    HostMap *m = (HostMap *)p;
    m->map->mergeMapPoints(prevlmid, newlmid);
    return 0;
}

static void fill_match_job(HostMap *m, int kfid, int n_local, const int *local, MatchJob &J)
{
    J.pmap = m->map.get(); J.kfid = kfid;
    J.set_local_lmids.insert(local, local + n_local);
}

// what Mapper::matchToMap assembles for keyframe kfid and the local set `local` in front of its matcher
// (SlamManager::assembleMatchToMap), no GPU context needed: kp_lmid (cap) the keypoints offered, in grid order; cand_lmid (cap)
// the candidates offered, in the iteration order of the set; n[2] = their counts (both 0 when there is nothing to match).
// OV2_ERR_INVALID when the keyframe is not in the map or a count exceeds cap
int ov2h_match_assemble(void *p, int kfid, int n_local, const int *local, int cap, int *n, int *kp_lmid, int *cand_lmid)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f || n_local < 0) return (int)OV2_ERR_INVALID;
    MatchJob J;
    fill_match_job(m, kfid, n_local, local, J);
    SlamManager::assembleMatchToMap(*f, J.set_local_lmids, J);
    n[0] = J.offered ? (int)J.kp_lmid.size() : 0; n[1] = J.offered ? (int)J.cand_lmid.size() : 0;
    if (n[0] > cap || n[1] > cap) return (int)OV2_ERR_INVALID;
    std::copy(J.kp_lmid.begin(), J.kp_lmid.begin() + n[0], kp_lmid);
    std::copy(J.cand_lmid.begin(), J.cand_lmid.begin() + n[1], cand_lmid);
    return 0;
}

// SlamManager::matchToLocalMaps on B maps of one context: keyframe kfid[b] of maps[b] against the n_local[b] lmids of map b,
// one list after the other in `local`, with the two gates of Mapper::matchToMap; merge: MapManager::mergeMapPoints per pair
// afterwards; single: one ov2_match_to_map call per job instead of one ov2_match_to_map_batch call.  pairs (cap x 2): the
// (previous lmid, new lmid) pairs job after job, ascending previous lmid, n_pairs[b] each; stats[5]: jobs, jobs offered,
// keypoints offered, candidates offered, library calls.  Returns 0 or a negative ov2_status (OV2_ERR_INVALID also when cap
// is too small)
static int match_local_maps_impl(int B, void *const *maps, void *ctx, const int *kfid, const int *n_local, const int *local, float fmaxprojerr,
                                 float fdistratio, int merge, int single, int cap, int *n_pairs, int *pairs, int *stats, bool mirror);

int ov2h_match_local_maps(int B, void *const *maps, void *ctx, const int *kfid, const int *n_local, const int *local, float fmaxprojerr,
                          float fdistratio, int merge, int single, int cap, int *n_pairs, int *pairs, int *stats)
{
    return match_local_maps_impl(B, maps, ctx, kfid, n_local, local, fmaxprojerr, fdistratio, merge, single, cap, n_pairs, pairs, stats, false);
}

// the same with the mirror path asked for (SlamManager::matchToLocalMaps(..., mirror = true)): taken when every map has a device
// mirror with the match columns
int ov2h_match_local_maps_mirror(int B, void *const *maps, void *ctx, const int *kfid, const int *n_local, const int *local, float fmaxprojerr,
                                 float fdistratio, int merge, int single, int cap, int *n_pairs, int *pairs, int *stats)
{
    return match_local_maps_impl(B, maps, ctx, kfid, n_local, local, fmaxprojerr, fdistratio, merge, single, cap, n_pairs, pairs, stats, true);
}

static int match_local_maps_impl(int B, void *const *maps, void *ctx, const int *kfid, const int *n_local, const int *local, float fmaxprojerr,
                                 float fdistratio, int merge, int single, int cap, int *n_pairs, int *pairs, int *stats, bool mirror)
{
    if (B < 0) return (int)OV2_ERR_INVALID;
    std::vector<MatchJob> jobs((size_t)B);
    size_t o = 0;
    for (int b = 0; b < B; ++b) {
        if (!maps[b] || n_local[b] < 0) return (int)OV2_ERR_INVALID;
        fill_match_job((HostMap *)maps[b], kfid[b], n_local[b], local + o, jobs[b]);
        o += (size_t)n_local[b];
    }
    MatchBatchStats st;
    const ov2_status s = SlamManager::matchToLocalMaps((ov2_ctx *)ctx, jobs, fmaxprojerr, fdistratio, merge != 0, single != 0, st, mirror);
    const int sv[5] = {st.jobs, st.match_jobs, st.n_kp, st.n_cand, st.match_calls};
    std::copy(sv, sv + 5, stats);
    if (s != OV2_OK) return (int)s;
    o = 0;
    for (int b = 0; b < B; ++b) {
        const auto &mp = jobs[b].map_previd_newid;
        if (o + mp.size() > (size_t)cap) return (int)OV2_ERR_INVALID;
        n_pairs[b] = (int)mp.size();
        for (const auto &q : mp) { pairs[2 * o] = q.first; pairs[2 * o + 1] = q.second; ++o; }
    }
    return 0;
}

// LoopCloser::processLoopCandidates on B pairs: branch (B, ov2::LoopBranch of the 2D-2D half), n_passed (B: pairs it passed on),
// then the rows of ov2h_loop_verify (a pair that did not pass keeps the row of an untouched LoopVerifyResult); stats[13]: the five
// of ov2h_loop_match followed by the eight of ov2h_loop_verify
int ov2h_loop_process(void *p, void *ctx, int B, const int *newkf, const int *lckf, const unsigned long long *seeds, int nransac_iter,
                      float fransac_err, int cap, int *branch, int *n_passed, int *ints, double *dbl, int *lists, int *stats)
{
    HostMap *m = (HostMap *)p;
    if (B < 0) return (int)OV2_ERR_INVALID;
    loop_params(m, nransac_iter, fransac_err);
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> pairs((size_t)B);
    std::vector<uint64_t> sd((size_t)B);
    for (int b = 0; b < B; ++b) { pairs[b] = {newkf[b], lckf[b]}; sd[b] = (uint64_t)seeds[b]; }
    std::vector<LoopPairResult> matched;
    std::vector<LoopVerifyResult> out;
    const ov2_status s = lc.processLoopCandidates(pairs, sd, matched, out);
    if (s != OV2_OK) return (int)s;
    size_t used = 0;
    for (int b = 0; b < B; ++b) {
        branch[b] = matched[b].branch; n_passed[b] = (int)matched[b].vkplmids.size();
        if (!pack_verify(out[b], ints + 13 * b, dbl + 15 * b, cap, lists, &used)) return (int)OV2_ERR_INVALID;
    }
    const LoopStats &L = lc.last_;
    const int st[13] = {L.pairs, L.knn_pairs, L.epi_pairs, L.knn_calls, L.epi_calls, L.p3p_pairs, L.refine_pairs, L.track_pairs, L.pnp_pairs,
                        L.p3p_calls, L.refine_calls, L.track_calls, L.pnp_calls};
    std::copy(st, st + 13, stats);
    return 0;
}

// LoopCloser::acceptMatch (the ratio test of knnMatching, :434-442); d1 < 0 = fewer than two neighbours
int ov2h_loop_accept(int d0, int d1) { return LoopCloser::acceptMatch(d0, d1) ? 1 : 0; }

// LoopCloser::removeOutliers (:899-928) on n pairs with n_out outlier indices; pairs (n x 2) is rewritten in place; returns
// the number of pairs left
int ov2h_loop_remove_outliers(int n, int *pairs, int n_out, const int *outliers)
{
    std::vector<std::pair<int, int>> v((size_t)n);
    for (int i = 0; i < n; ++i) v[i] = {pairs[2 * i], pairs[2 * i + 1]};
    std::vector<int> o(outliers, outliers + n_out);
    LoopCloser::removeOutliers(v, o);
    for (size_t i = 0; i < v.size(); ++i) { pairs[2 * i] = v[i].first; pairs[2 * i + 1] = v[i].second; }
    return (int)v.size();
}

// LoopCloser::processLoopCandidate (:184-236 as written, one pair, a launch and a synchronisation per stage).  out[5]: branch,
// candidate used, pairs before the filter, outliers, pairs after it; success: the filter's bool (-1 = not reached);
// pairs_knn / pairs_out (cap x 2): the two lists.  Returns 0 or a negative ov2_status
int ov2h_loop_candidate(void *p, void *ctx, int newkf, int lckf, unsigned long long seed, int nransac_iter, float fransac_err, int cap,
                        int *out, int *success, int *pairs_knn, int *pairs_out)
{
    HostMap *m = (HostMap *)p;
    m->st->nransac_iter_ = nransac_iter; m->st->fransac_err_ = fransac_err;
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    LoopPairResult r;
    const ov2_status s = lc.processLoopCandidate(newkf, lckf, (uint64_t)seed, r);
    if (s != OV2_OK) return (int)s;
    if (r.vkplmids_knn.size() > (size_t)cap) return (int)OV2_ERR_INVALID;
    out[0] = r.branch; out[1] = r.lckfid; out[2] = (int)r.vkplmids_knn.size(); out[3] = r.n_outliers; out[4] = (int)r.vkplmids.size();
    *success = r.epi_status;
    for (size_t i = 0; i < r.vkplmids_knn.size(); ++i) { pairs_knn[2 * i] = r.vkplmids_knn[i].first; pairs_knn[2 * i + 1] = r.vkplmids_knn[i].second; }
    for (size_t i = 0; i < r.vkplmids.size(); ++i) { pairs_out[2 * i] = r.vkplmids[i].first; pairs_out[2 * i + 1] = r.vkplmids[i].second; }
    return 0;
}

// LoopCloser::matchLoopCandidates on B pairs (newkf[b], lckf[b]) with one sampler seed each; nransac_iter / fransac_err as the
// YAML keys.  Per pair: branch (ov2::LoopBranch); counts (B x 8): candidate used, identity pairs, query rows, train rows, pairs
// before the filter, outliers, pairs after the filter, epipolar status (-1 = not offered); info (B x 4): the filter's info; Rt
// (B x 12): R then t where the status is >= 1.  pairs_knn / pairs_out (cap x 2 each): the lists before / after the filter,
// pair after pair.  stats[5]: pairs, offered to the matcher, offered to the filter, matcher launches, filter launches.
// Returns 0 or a negative ov2_status (OV2_ERR_INVALID also when cap is too small)
int ov2h_loop_match(void *p, void *ctx, int B, const int *newkf, const int *lckf, const unsigned long long *seeds, int nransac_iter,
                    float fransac_err, int cap, int *branch, int *counts, int *info, double *Rt, int *pairs_knn, int *pairs_out,
                    int *stats)
{
    HostMap *m = (HostMap *)p;
    m->st->nransac_iter_ = nransac_iter; m->st->fransac_err_ = fransac_err;
    LoopCloser lc((ov2_ctx *)ctx, m->st, m->map);
    std::vector<std::pair<int, int>> pairs((size_t)B);
    std::vector<uint64_t> sd((size_t)B);
    for (int b = 0; b < B; ++b) { pairs[b] = {newkf[b], lckf[b]}; sd[b] = (uint64_t)seeds[b]; }
    std::vector<LoopPairResult> out;
    const ov2_status s = lc.matchLoopCandidates(pairs, sd, out);
    if (s != OV2_OK) return (int)s;
    size_t ok = 0, oo = 0;
    for (int b = 0; b < B; ++b) {
        const LoopPairResult &r = out[b];
        if (ok + r.vkplmids_knn.size() > (size_t)cap || oo + r.vkplmids.size() > (size_t)cap) return (int)OV2_ERR_INVALID;
        branch[b] = r.branch;
        int *c = counts + 8 * b;
        c[0] = r.lckfid; c[1] = r.n_identity; c[2] = r.n_query; c[3] = r.n_train; c[4] = (int)r.vkplmids_knn.size();
        c[5] = r.n_outliers; c[6] = (int)r.vkplmids.size(); c[7] = r.epi_status;
        std::copy(r.epi_info, r.epi_info + 4, info + 4 * b);
        std::copy(r.R, r.R + 9, Rt + 12 * b); std::copy(r.t, r.t + 3, Rt + 12 * b + 9);
        for (const auto &q : r.vkplmids_knn) { pairs_knn[2 * ok] = q.first; pairs_knn[2 * ok + 1] = q.second; ++ok; }
        for (const auto &q : r.vkplmids) { pairs_out[2 * oo] = q.first; pairs_out[2 * oo + 1] = q.second; ++oo; }
    }
    stats[0] = lc.last_.pairs; stats[1] = lc.last_.knn_pairs; stats[2] = lc.last_.epi_pairs; stats[3] = lc.last_.knn_calls;
    stats[4] = lc.last_.epi_calls;
    return 0;
}

// The bookkeeping of a host map that ov2h_map_export does not show, as flat lists (call with zero capacities for the sizes
// n[3]): per landmark (lmid, MapPoint::kfid_, is3d_, isobs_), the observer sets as (lmid, kfid) pairs, and Frame::map_covkfs_
// of every keyframe as (kfid, covisible kfid, count) triples
int ov2h_map_export_graph(void *p, int cap_lm, int cap_obs, int cap_cov, int *n, int *lm, int *observers, int *cov)
{
    const MapManager &M = *((HostMap *)p)->map;
    int nl = 0, no = 0, nc = 0;
    for (const auto &kv : M.map_plms_) {
        const MapPoint &q = *kv.second;
        if (nl < cap_lm) { lm[4 * nl] = kv.first; lm[4 * nl + 1] = q.kfid_; lm[4 * nl + 2] = q.is3d_; lm[4 * nl + 3] = q.isobs_; }
        ++nl;
        for (int k : q.set_kfids_) { if (no < cap_obs) { observers[2 * no] = kv.first; observers[2 * no + 1] = k; } ++no; }
    }
    for (const auto &kv : M.map_pkfs_)
        for (const auto &c : kv.second->map_covkfs_) {
            if (nc < cap_cov) { cov[3 * nc] = kv.first; cov[3 * nc + 1] = c.first; cov[3 * nc + 2] = c.second; }
            ++nc;
        }
    n[0] = nl; n[1] = no; n[2] = nc;
    return 0;
}

// MapPoint::invdepth_ of a landmark (-1: never set, or no such landmark)
double ov2h_landmark_invdepth(void *p, int lmid)
{
    auto lm = ((HostMap *)p)->map->getMapPoint(lmid);
    return lm ? lm->invdepth_ : -1.;
}

int ov2h_set_params(void *p, int klt_use_prior, int stereo_rect, int nklt_pyr_lvl, int nklt_win_size)
{
    HostMap *m = (HostMap *)p;
    m->st->klt_use_prior_ = klt_use_prior != 0; m->st->bdo_stereo_rect_ = stereo_rect != 0;
    m->st->nklt_pyr_lvl_ = nklt_pyr_lvl; m->st->nklt_win_size_ = nklt_win_size;
    return 0;
}

// dop3p / nransac_iter / fransac_err / bdo_random of the YAML for the P3P stage of computePose + the sampler's base seed;
// clears a pending P3P request
int ov2h_set_p3p(void *p, int dop3p, int nransac_iter, float fransac_err, int bdo_random, unsigned long long seed)
{
    HostMap *m = (HostMap *)p;
    m->st->dop3p_ = dop3p != 0; m->st->nransac_iter_ = nransac_iter; m->st->fransac_err_ = fransac_err;
    m->st->bdo_random_ = bdo_random != 0; m->st->epi_seed_ = (uint64_t)seed;
    m->bp3preq = false;
    return 0;
}

// out[5]: what the P3P branch did in the last ov2h_compute_pose: ran, p3pRansac's return, correspondences in, observations
// removed before ceresPnP, 1 if the frame ended in resetFrame()
void ov2h_p3p_stats(void *p, double *out)
{
    const P3pStats &e = ((HostMap *)p)->last_p3p;
    out[0] = e.ran; out[1] = e.status; out[2] = e.points; out[3] = e.removed; out[4] = e.reset;
}

// MapManager::stereoMatching(frame, vleftpyr, vrightpyr) on keyframe kfid; the two pyramids are built here the way
// Mapper::run does (src/mapper.cpp:76-81: CLAHE + buildOpticalFlowPyramid of the right image; the left one is the frame's)
int ov2h_stereo_matching(void *p, void *ctx, int kfid, const uint8_t *img_left, const uint8_t *img_right, int w, int h)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    ov2_ctx *c = (ov2_ctx *)ctx;
    ov2_pyr *pl = nullptr, *pr = nullptr;
    const SlamParams &st = *m->st;
    ov2_status s = ov2_pyramid_build(c, img_left, w, h, w, st.nklt_win_size_, st.nklt_pyr_lvl_, st.use_clahe_ ? 1 : 0, st.fclahe_val_,
                                     w / 50, h / 50, &pl);
    if (s != OV2_OK) return s;
    Pyramid L(pl);
    s = ov2_pyramid_build(c, img_right, w, h, w, st.nklt_win_size_, st.nklt_pyr_lvl_, st.use_clahe_ ? 1 : 0, st.fclahe_val_, w / 50,
                          h / 50, &pr);
    if (s != OV2_OK) return s;
    Pyramid R(pr);
    FeatureTracker tracker(c, st.nmax_iter_, st.fmax_px_precision_);
    return m->map->stereoMatching(*f, L, R, tracker, st);
}

// VisualFrontEnd::preprocessImage (twice: previous image, current image) + kltTracking with keyframe kfid as the
// current frame (its keypoints sit at their previous-image positions, as at src/visual_front_end.cpp:132)
int ov2h_klt_tracking(void *p, void *ctx, int kfid, const uint8_t *img_prev, const uint8_t *img_cur, int w, int h, int *p3p_req)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    ov2_ctx *c = (ov2_ctx *)ctx;
    m->map->pcurframe_ = f;
    auto tracker = std::make_shared<FeatureTracker>(c, m->st->nmax_iter_, m->st->fmax_px_precision_);
    VisualFrontEnd fe(c, m->st, f, m->map, tracker);
    ov2_status s = fe.preprocessImage(img_prev, w, h, w);
    if (s != OV2_OK) return s;
    if ((s = fe.preprocessImage(img_cur, w, h, w)) != OV2_OK) return s;
    s = fe.kltTracking();
    if (p3p_req) *p3p_req = fe.bp3preq_ ? 1 : 0;
    return s;
}

// keypoints of keyframe kfid: lmid, px, is3d, is_stereo, rpx (arrays of capacity cap); returns the count
int ov2h_get_keypoints(void *p, int kfid, int cap, int *lmid, float *px, uint8_t *is3d, uint8_t *is_stereo, float *rpx)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    int n = 0;
    for (const auto &kv : f->mapkps_) {
        if (n < cap) {
            const Keypoint &k = kv.second;
            lmid[n] = k.lmid_; px[2 * n] = k.px_.x; px[2 * n + 1] = k.px_.y; is3d[n] = k.is3d_; is_stereo[n] = k.is_stereo_;
            rpx[2 * n] = k.rpx_.x; rpx[2 * n + 1] = k.rpx_.y;
        }
        ++n;
    }
    return n;
}

// Frame::projWorldToRightImageDist / projWorldToImage of keyframe kfid (test hook)
int ov2h_project(void *p, int kfid, const double *xyz, int right, float *px)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    const Point2f q = right ? f->projWorldToRightImageDist(Vec3{xyz[0], xyz[1], xyz[2]}) : f->projWorldToImage(Vec3{xyz[0], xyz[1], xyz[2]});
    px[0] = q.x; px[1] = q.y;
    return 0;
}

// CameraCalibration::Dcv_ / model_ of the left (cam = 0) or right camera: model 0 = pinhole (k1 k2 p1 p2 [k3]), 1 = fisheye (k1..k4)
int ov2h_set_distortion(void *p, int cam, int model, int n, const double *coeffs)
{
    HostMap *m = (HostMap *)p;
    auto &c = cam ? m->cr : m->cl;
    if (!c || n < 0 || n > 5) return -1;
    c->model_ = model ? CameraCalibration::Fisheye : CameraCalibration::Pinhole;
    c->D_.assign(coeffs, coeffs + n);
    return 0;
}

// CameraCalibration::undistortImagePoint / projectCamToImageDist (test hooks)
int ov2h_undistort(void *p, int cam, float x, float y, float *out)
{
    HostMap *m = (HostMap *)p;
    const auto &c = cam ? m->cr : m->cl;
    if (!c) return -1;
    const Point2f q = c->undistortImagePoint(Point2f{x, y});
    out[0] = q.x; out[1] = q.y;
    return 0;
}

int ov2h_project_dist(void *p, int cam, const double *pc, float *out)
{
    HostMap *m = (HostMap *)p;
    const auto &c = cam ? m->cr : m->cl;
    if (!c) return -1;
    const Point2f q = c->projectCamToImageDist(Vec3{pc[0], pc[1], pc[2]});
    out[0] = q.x; out[1] = q.y;
    return 0;
}

int ov2h_get_frl(void *p, int kfid, double *F9)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    for (int i = 0; i < 9; ++i) F9[i] = f->Frl_[i];
    return 0;
}

int ov2h_map_finalize(void *p, int newkf)
{
    HostMap *m = (HostMap *)p;
    for (auto &kv : m->map->map_pkfs_) m->map->updateFrameCovisibility(*kv.second);
    m->map->pcurframe_ = m->map->getKeyframe(newkf);
    return m->map->pcurframe_ ? 0 : -1;
}

int ov2h_local_ba_setup(void *p, int newkf, int *n_pose, int *n_lm, int *n_res)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f) return -1;
    Optimizer opt(nullptr, m->st, m->map);
    m->pb = LocalBAProblem();
    opt.setupLocalBA(*f, m->pb);
    *n_pose = (int)m->pb.pose_const.size(); *n_lm = (int)m->pb.lm_lmid.size(); *n_res = (int)m->pb.res_type.size();
    return m->pb.aborted ? 1 : 0;
}

// device map mirror: walk the host map once into an ov2_map; later set-ups (and ov2h_apply_local_ba) use it
int ov2h_map_attach_device(void *p, void *ctx, int max_kf, int max_lm, int max_obs)
{
    HostMap *m = (HostMap *)p;
    return (int)m->map->attachDevice((ov2_ctx *)ctx, max_kf, max_lm, max_obs);
}

// MapManager::enableMatchColumns: the mirror keeps Keypoint::px_ and the descriptors from here on
int ov2h_map_enable_match_columns(void *p) { return (int)((HostMap *)p)->map->enableMatchColumns(); }

// the ov2_map behind the host map (tests compare its tables with a map updated on the device)
void *ov2h_map_device_handle(void *p) { return ((HostMap *)p)->map->dev_; }

// MapManager::flushDevice: push the queued edits of the host objects to the device mirror
int ov2h_map_flush_device(void *p) { return (int)((HostMap *)p)->map->flushDevice(); }

// rows / capacity / compactions of the device mirror's observation table (ov2_map_obs_rows)
int ov2h_map_device_rows(void *p, int *rows, int *capacity, int *compactions)
{
    HostMap *m = (HostMap *)p;
    if (!m->map->dev_) return -1;
    return (int)ov2_map_obs_rows(m->map->dev_, rows, capacity, compactions);
}

int ov2h_local_ba_setup_dev(void *p, int newkf, int *n_pose, int *n_lm, int *n_res)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f || !m->map->dev_) return -1;
    Optimizer opt(nullptr, m->st, m->map);
    m->pb = LocalBAProblem();
    if (opt.setupLocalBADevice(*f, m->pb) != OV2_OK) return -2;
    *n_pose = (int)m->pb.pose_const.size(); *n_lm = (int)m->pb.lm_lmid.size(); *n_res = (int)m->pb.res_type.size();
    return m->pb.aborted ? 1 : 0;
}

// test hooks for the incremental path: mutate the host map through the MapManager (which queues the device edits)
int ov2h_map_remove_obs(void *p, int kfid, int lmid) { ((HostMap *)p)->map->removeMapPointObs(lmid, kfid); return 0; }
int ov2h_map_remove_landmark(void *p, int lmid) { ((HostMap *)p)->map->removeMapPoint(lmid); return 0; }
int ov2h_map_set_isobs(void *p, int lmid, int isobs)
{
    HostMap *m = (HostMap *)p;
    auto plm = m->map->getMapPoint(lmid);
    if (!plm) return -1;
    plm->isobs_ = isobs != 0;
    m->map->touchMapPoint(lmid);
    return 0;
}
int ov2h_map_bad_lmids(void *p, int *out, int cap)
{
    HostMap *m = (HostMap *)p;
    int n = 0;
    for (int l : m->pb.set_badlmids) { if (n < cap) out[n] = l; ++n; }
    return n;
}

// ---- the local BA in its three stages on the host objects, so that the map can be edited between set-up and update (the
// reference's other threads keep working while Optimizer::localBA solves without the map lock, src/optimizer.cpp:741)
static Keypoint make_kp(int lmid, const float *uv, int is_stereo, const float *ruv)
{
    Keypoint kp;
    kp.lmid_ = lmid; kp.px_ = {uv[0], uv[1]}; kp.unpx_ = {uv[0], uv[1]}; kp.is3d_ = true;
    kp.is_stereo_ = is_stereo != 0;
    if (kp.is_stereo_) { kp.rpx_ = {ruv[0], ruv[1]}; kp.runpx_ = {ruv[0], ruv[1]}; }
    return kp;
}

// solves the problem the last ov2h_local_ba_setup left, in place, as Optimizer::localBA's host branch does (robust solve +
// flags + L2 refinement through ov2_ba_solve); outlier: n_res bytes out (may be NULL)
int ov2h_local_ba_solve(void *p, void *ctx, int newkf, uint8_t *outlier, int *n_out1, int *n_out2)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f || m->pb.aborted) return -1;
    ov2_ba_problem pr = m->pb.view(*m->st, *f);
    ov2_ba_options o;
    ov2_ba_default_options(&o, m->st->robust_mono_th_);
    o.l2_refine = m->st->apply_l2_after_robust_ ? 1 : 0;
    std::vector<double> chi2(pr.n_res);
    std::vector<uint8_t> depth(pr.n_res), flags(pr.n_res);
    ov2_ba_result r;
    std::memset(&r, 0, sizeof(r));
    r.chi2 = chi2.data(); r.depth_positive = depth.data(); r.outlier = flags.data();
    const ov2_status s = ov2_ba_solve((ov2_ctx *)ctx, &pr, &o, &r);
    if (s != OV2_OK) return (int)s;
    if (outlier) std::copy(flags.begin(), flags.end(), outlier);
    if (n_out1) *n_out1 = r.n_outliers_pass1;
    if (n_out2) *n_out2 = r.n_outliers_pass2;
    return 0;
}

// Optimizer::updateAfterLocalBA (:741-882) on that problem (its pose / lm arrays: as set up, or as ov2h_local_ba_solve left
// them) with the given per residual block flags, against the map as it is now.  No GPU.
int ov2h_local_ba_update(void *p, int newkf, int n_res, const uint8_t *outlier, int cur_frame_obs)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f || m->pb.aborted || n_res != (int)m->pb.res_type.size() || (n_res && !outlier)) return -1;
    ov2_ba_result r;
    std::memset(&r, 0, sizeof(r));
    r.outlier = const_cast<uint8_t *>(outlier);
    Optimizer opt(nullptr, m->st, m->map);
    opt.updateAfterLocalBA(*f, m->pb, r, cur_frame_obs != 0);
    return 0;
}

// a new keyframe with n observations of existing landmarks (MapManager::addKeyframe); uv / ruv: n x 2
int ov2h_map_add_keyframe_obs(void *p, int kfid, const double *Twc7, int n, const int *lmid, const float *uv, const uint8_t *is_stereo,
                              const float *ruv)
{
    HostMap *m = (HostMap *)p;
    if (m->map->getKeyframe(kfid)) return -1;
    auto f = std::make_shared<Frame>();
    f->id_ = kfid; f->kfid_ = kfid;
    f->pcalib_leftcam_ = m->cl; f->pcalib_rightcam_ = m->cr;
    SE3 T;
    for (int i = 0; i < 7; ++i) T.v[i] = Twc7[i];
    f->setTwc(T);
    for (int i = 0; i < n; ++i) {
        if (!m->map->getMapPoint(lmid[i])) return -1;
        f->addKeypoint(make_kp(lmid[i], uv + 2 * i, is_stereo[i], ruv + 2 * i));
    }
    return (int)m->map->addKeyframe(f);
}

// n more observations by the existing keyframe kfid (MapManager::addMapPointKfObs: the matchToMap / merge path)
int ov2h_map_append_obs(void *p, int kfid, int n, const int *lmid, const float *uv, const uint8_t *is_stereo, const float *ruv)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    for (int i = 0; i < n; ++i) {
        if (!m->map->getMapPoint(lmid[i]) || f->isObservingKp(lmid[i])) return -1;
        m->map->addMapPointKfObs(kfid, make_kp(lmid[i], uv + 2 * i, is_stereo[i], ruv + 2 * i));
    }
    return 0;
}

// the whole host map keyed by ids, comparable with the device tables: live keyframe poses, live landmarks (point + OV2_LM_*
// bits), live (kfid, lmid) observations (Frame::mapkps_ entries whose map point exists) with their stereo flag.  Returns
// the three counts in n[3]; arrays are written up to their capacities (call with zero capacities for the sizes).
int ov2h_map_export(void *p, int cap_kf, int cap_lm, int cap_obs, int *n, int *kf_id, double *kf_pose, int *lm_id, double *lm_xyz,
                    uint8_t *lm_state, int *obs_kf, int *obs_lm, uint8_t *obs_stereo)
{
    HostMap *m = (HostMap *)p;
    const MapManager &M = *m->map;
    int nk = 0, nl = 0, no = 0;
    for (const auto &kv : M.map_pkfs_) {
        if (!kv.second) continue;
        if (nk < cap_kf) {
            kf_id[nk] = kv.first;
            const SE3 T = kv.second->getTwc();
            for (int i = 0; i < 7; ++i) kf_pose[7 * nk + i] = T.v[i];
        }
        ++nk;
        for (const auto &kp : kv.second->mapkps_) {
            if (!M.getMapPoint(kp.first)) continue;
            if (no < cap_obs) { obs_kf[no] = kv.first; obs_lm[no] = kp.first; obs_stereo[no] = kp.second.is_stereo_ ? 1 : 0; }
            ++no;
        }
    }
    for (const auto &kv : M.map_plms_) {
        if (!kv.second) continue;
        if (nl < cap_lm) {
            lm_id[nl] = kv.first;
            const Vec3 x = kv.second->getPoint();
            lm_xyz[3 * nl] = x.x; lm_xyz[3 * nl + 1] = x.y; lm_xyz[3 * nl + 2] = x.z;
            lm_state[nl] = M.lmState(*kv.second);
        }
        ++nl;
    }
    n[0] = nk; n[1] = nl; n[2] = no;
    return 0;
}

int ov2h_local_ba_get(void *p, int *pose_kfid, uint8_t *pose_const, double *pose, int *lm_lmid, double *lm,
                      int *lm_anchor_kfid, double *lm_anchor_uv, uint8_t *res_type, int *res_kfid, int *res_lmid,
                      double *res_uv)
{
    HostMap *m = (HostMap *)p;
    const LocalBAProblem &pb = m->pb;
    const int e = m->st->buse_inv_depth_ ? 1 : 3;
    for (size_t i = 0; i < pb.pose_const.size(); ++i) { pose_kfid[i] = pb.pose_kfid[i]; pose_const[i] = pb.pose_const[i]; }
    std::memcpy(pose, pb.pose.data(), pb.pose.size() * sizeof(double));
    for (size_t i = 0; i < pb.lm_lmid.size(); ++i) {
        lm_lmid[i] = pb.lm_lmid[i];
        lm_anchor_kfid[i] = pb.lm_anchor_pose[i] >= 0 ? pb.pose_kfid[pb.lm_anchor_pose[i]] : -1;
        lm_anchor_uv[2 * i] = pb.lm_anchor_uv[2 * i]; lm_anchor_uv[2 * i + 1] = pb.lm_anchor_uv[2 * i + 1];
        for (int c = 0; c < e; ++c) lm[i * e + c] = pb.lm[i * e + c];
    }
    for (size_t i = 0; i < pb.res_type.size(); ++i) {
        res_type[i] = pb.res_type[i]; res_kfid[i] = pb.pose_kfid[pb.res_pose[i]]; res_lmid[i] = pb.lm_lmid[pb.res_lm[i]];
        res_uv[2 * i] = pb.res_uv[2 * i]; res_uv[2 * i + 1] = pb.res_uv[2 * i + 1];
    }
    return 0;
}

// Estimator::applyLocalBA on the GPU context `ctx` (an ov2_ctx*)
int ov2h_apply_local_ba(void *p, void *ctx, int newkf, int *n_outliers1, int *n_outliers2, double *final_cost)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f) return -1;
    auto opt = std::make_shared<Optimizer>((ov2_ctx *)ctx, m->st, m->map);
    Estimator est(m->st, m->map, opt);
    est.pnewkf_ = f;
    const ov2_status s = est.applyLocalBA();
    if (n_outliers1) *n_outliers1 = opt->last_result_.n_outliers_pass1;
    if (n_outliers2) *n_outliers2 = opt->last_result_.n_outliers_pass2;
    if (final_cost) *final_cost = opt->last_result_.l2_done ? opt->last_result_.l2_final_cost : opt->last_result_.final_cost;
    return s;
}

// Optimizer::structureOnlyBA(vlm2optids) on the GPU context `ctx`
int ov2h_structure_only_ba(void *p, void *ctx, int n, const int *lmids, double *final_cost, int *n_iters)
{
    HostMap *m = (HostMap *)p;
    Optimizer opt((ov2_ctx *)ctx, m->st, m->map);
    const ov2_status s = opt.structureOnlyBA(std::vector<int>(lmids, lmids + n));
    if (final_cost) *final_cost = opt.last_result_.final_cost;
    if (n_iters) *n_iters = opt.last_result_.n_log - 1;
    return s;
}

// set-up stage shared by Optimizer::fullBA / looseBA (keyframes kf_lo .. kf_hi, observers above kf_obs_max ignored,
// landmarks with fewer than min_obs observers set aside); read back with ov2h_local_ba_get
int ov2h_range_ba_setup(void *p, int kf_lo, int kf_hi, int kf_obs_max, int min_obs, int *n_pose, int *n_lm, int *n_res)
{
    HostMap *m = (HostMap *)p;
    Optimizer opt(nullptr, m->st, m->map);
    m->pb = LocalBAProblem();
    opt.setupRangeBA(kf_lo, kf_hi, kf_obs_max, (size_t)min_obs, m->pb);
    *n_pose = (int)m->pb.pose_const.size(); *n_lm = (int)m->pb.lm_lmid.size(); *n_res = (int)m->pb.res_type.size();
    return 0;
}

// Optimizer::fullBA(buse_robust_cost) on the GPU context `ctx`
int ov2h_full_ba(void *p, void *ctx, int robust, int *n_out1, int *n_out2, double *final_cost, int *n_iters)
{
    HostMap *m = (HostMap *)p;
    Optimizer opt((ov2_ctx *)ctx, m->st, m->map);
    const ov2_status s = opt.fullBA(robust != 0);
    const ov2_ba_result &r = opt.last_result_;
    if (n_out1) *n_out1 = r.n_outliers_pass1;
    if (n_out2) *n_out2 = r.n_outliers_pass2;
    if (final_cost) *final_cost = r.l2_done ? r.l2_final_cost : r.final_cost;
    if (n_iters) *n_iters = r.n_log;
    return s;
}

// Optimizer::looseBA(inikfid, nkfid, buse_robust_cost)
int ov2h_loose_ba(void *p, void *ctx, int inikfid, int nkfid, int robust, int *n_out1, double *final_cost)
{
    HostMap *m = (HostMap *)p;
    Optimizer opt((ov2_ctx *)ctx, m->st, m->map);
    const ov2_status s = opt.looseBA(inikfid, nkfid, robust != 0);
    if (n_out1) *n_out1 = opt.last_result_.n_outliers_pass1;
    if (final_cost) *final_cost = opt.last_result_.final_cost;
    return s;
}

// MapManager::removeKeyframe(kfid): its observations leave their map points, its covisibility entries go; with a mirror
// attached the removal reaches it at once (ov2_map_remove_keyframe)
int ov2h_map_remove_keyframe(void *p, int kfid)
{
    return (int)((HostMap *)p)->map->removeKeyframe(kfid);
}

// MapManager::pcurframe_ as a live sequence has it: a Frame of its own that carries keyframe kfid's id, pose and keypoints
// (ov2h_map_finalize makes the newest keyframe OBJECT the current frame, which then takes every current-frame update on
// top of its keyframe update); kfid < 0: no current frame
int ov2h_map_set_cur_frame(void *p, int kfid)
{
    HostMap *m = (HostMap *)p;
    if (kfid < 0) { m->map->pcurframe_ = nullptr; return 0; }
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    m->map->pcurframe_ = std::make_shared<Frame>(*f);
    return 0;
}

// Optimizer::applyLooseBA alone: the assembly of looseBA(inikfid, nkfid, .), then the free poses (n_pose x 7), the landmarks
// (n_lm x 1 or 3) and the per-block flags (n_res bytes) of the flat problem are overwritten with the given arrays -- in the
// order ov2h_range_ba_setup(inikfid, nkfid, nkfid, 0) lists them -- and the update stage runs.  Needs no GPU context.
// T_corr7 (may be NULL): opt * inverse(old(nkfid)), the correction of the loop keyframe, as the stage formed it.
// returns 1 ran, 0 no-op (no residual block), < 0 error (-1 nkfid not alive, -2 the sizes are not those of the problem)
int ov2h_apply_loose_ba(void *p, int inikfid, int nkfid, int n_pose, const double *pose, int n_lm, const double *lm, int n_res,
                        const uint8_t *outlier, double *T_corr7)
{
    HostMap *m = (HostMap *)p;
    auto pnew = m->map->getKeyframe(nkfid);
    if (!pnew) return -1;
    Optimizer opt(nullptr, m->st, m->map);
    LocalBAProblem pb;
    opt.setupRangeBA(inikfid, nkfid, pnew->kfid_, 0, pb);
    if (pb.res_type.empty() || !pb.kfid_to_pose.count(pnew->kfid_)) return 0;
    if (n_pose != (int)pb.pose_const.size() || n_lm != (int)pb.lm_lmid.size() || n_res != (int)pb.res_type.size()) return -2;
    for (int i = 0; i < n_pose; ++i)
        if (!pb.pose_const[i]) std::copy(pose + 7 * (size_t)i, pose + 7 * (size_t)i + 7, pb.pose.begin() + 7 * (size_t)i);
    std::copy(lm, lm + pb.lm.size(), pb.lm.begin());
    SE3 T;
    opt.applyLooseBA(*pnew, pb, outlier, &T);
    if (T_corr7) std::copy(T.v.begin(), T.v.end(), T_corr7);
    return 1;
}

// Optimizer::localPoseGraph(newframe = keyframe newkf, kfloop_id, newTwc). returns 1 accepted, 0 rejected, < 0 error
int ov2h_local_pose_graph(void *p, void *ctx, int newkf, int kfloop_id, const double *newTwc7, double *final_cost, int *n_log)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f) return -1;
    SE3 T;
    for (int k = 0; k < 7; ++k) T.v[k] = newTwc7[k];
    Optimizer opt((ov2_ctx *)ctx, m->st, m->map);
    ov2_status s = OV2_OK;
    const bool ok = opt.localPoseGraph(*f, kfloop_id, T, &s);
    if (final_cost) *final_cost = opt.last_pg_.final_cost;
    if (n_log) *n_log = opt.last_pg_.n_log;
    return s != OV2_OK ? -2 : (ok ? 1 : 0);
}

// Optimizer::assembleLocalPoseGraph alone: the graph localPoseGraph(newframe = keyframe newkf, kfloop_id, newTwc) would solve.
// Needs no GPU context.  kfids / cst (cap), pose (cap x 7): the chain, loop keyframe first; ei / ej (cap), Tij (cap x 7): its
// n edges, the closing edge last.  returns n = poses = edges (>= 2), 0 no chain (a dead newkf included), -2 cap too small
int ov2h_assemble_local_pose_graph(void *p, int newkf, int kfloop_id, const double *newTwc7, int cap, int *kfids, double *pose,
                                   uint8_t *cst, int *ei, int *ej, double *Tij)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f) return 0;
    SE3 T;
    for (int k = 0; k < 7; ++k) T.v[k] = newTwc7[k];
    Optimizer opt(nullptr, m->st, m->map);
    LocalPoseGraph g;
    if (!opt.assembleLocalPoseGraph(*f, kfloop_id, T, g)) return 0;
    const int n = (int)g.kfids.size();
    if (n > cap || (int)g.ei.size() > cap) return -2;
    std::copy(g.kfids.begin(), g.kfids.end(), kfids);
    std::copy(g.pose.begin(), g.pose.end(), pose);
    std::copy(g.cst.begin(), g.cst.end(), cst);
    std::copy(g.ei.begin(), g.ei.end(), ei);
    std::copy(g.ej.begin(), g.ej.end(), ej);
    std::copy(g.Tij.begin(), g.Tij.end(), Tij);
    return n;
}

// Optimizer::applyLocalPoseGraph alone (test hook): the n free keyframes kfids (ascending, last = newkf) take the poses
// Twc7 as if a solve had produced them; the loop pose is taken equal to the new keyframe's pose, so the degenerate test
// passes.  returns 1 applied, 0 rejected, -1 a keyframe is missing
int ov2h_apply_local_pose_graph(void *p, int newkf, int n, const int *kfids, const double *Twc7)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(newkf);
    if (!f || n < 1 || kfids[n - 1] != newkf) return -1;
    LocalPoseGraph g;
    g.iniTcw = f->getTcw();
    g.newkfid = newkf;
    g.kfids.push_back(-1);                      // the constant loop keyframe: the update never looks at it
    g.pose.assign(7, 0.0);
    for (int i = 0; i < n; ++i) {
        if (!m->map->getKeyframe(kfids[i])) return -1;
        g.kfids.push_back(kfids[i]);
        g.pose.insert(g.pose.end(), Twc7 + 7 * (size_t)i, Twc7 + 7 * (size_t)i + 7);
    }
    for (int k = 0; k < 7; ++k) g.newTwc.v[k] = Twc7[7 * (size_t)(n - 1) + k];
    // the test maps stand one of their keyframes in as the current frame (ov2h_map_finalize); a live current frame is an
    // object of its own, so set the alias aside: it would be moved once as a keyframe and once more as the current frame
    auto cur = m->map->pcurframe_;
    if (cur && m->map->getKeyframe(cur->kfid_) == cur) m->map->pcurframe_ = nullptr;
    Optimizer opt(nullptr, m->st, m->map);
    const bool ok = opt.applyLocalPoseGraph(g);
    m->map->pcurframe_ = cur;
    return ok ? 1 : 0;
}

// Optimizer::fullPoseGraph(vTwc, vTpc, viskf) on flat arrays (n x 7, n x 7, n); vTwc is overwritten
int ov2h_full_pose_graph(void *p, void *ctx, int n, double *Twc7, const double *Tpc7, const unsigned char *iskf, double *final_cost)
{
    HostMap *m = (HostMap *)p;
    std::vector<SE3> vTwc((size_t)n), vTpc((size_t)n);
    std::vector<bool> viskf((size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 7; ++k) { vTwc[i].v[k] = Twc7[7 * (size_t)i + k]; vTpc[i].v[k] = Tpc7[7 * (size_t)i + k]; }
        viskf[i] = iskf[i] != 0;
    }
    Optimizer opt((ov2_ctx *)ctx, m->st, m->map);
    ov2_status s = OV2_OK;
    const bool ok = opt.fullPoseGraph(vTwc, vTpc, viskf, &s);
    if (final_cost) *final_cost = opt.last_pg_.final_cost;
    if (ok)
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 7; ++k) Twc7[7 * (size_t)i + k] = vTwc[i].v[k];
    return s != OV2_OK ? -2 : (ok ? 1 : 0);
}

// VisualFrontEnd::computePose on keyframe `kfid` taken as the current frame, starting from pose Twc7_init.  The P3P request
// (bp3preq_) is kept between calls, as the front-end keeps it between frames: a call that sets it makes the next one run
// the P3P branch (see ov2h_p3p_stats).
int ov2h_compute_pose(void *p, void *ctx, int kfid, const double *Twc7_init, int *p3p_req)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kfid);
    if (!f) return -1;
    SE3 T0;
    for (int i = 0; i < 7; ++i) T0.v[i] = Twc7_init[i];
    f->setTwc(T0);
    m->map->pcurframe_ = f;
    VisualFrontEnd fe((ov2_ctx *)ctx, m->st, f, m->map, nullptr);
    fe.bp3preq_ = m->bp3preq;
    const ov2_status s = fe.computePose(&m->last_p3p);
    m->bp3preq = fe.bp3preq_;
    if (p3p_req) *p3p_req = fe.bp3preq_ ? 1 : 0;
    return s;
}

// VisualFrontEnd::epipolar2d2dFiltering (:446-655) with keyframe kf_cur taken as the current frame and kf_prev as its previous
// keyframe, nransac_iter / fransac_err as the YAML keys, bdo_random off (seed used as is).  removed[cap]: the ids the stage
// removed from kf_cur, ascending; stats[4] (may be NULL): as ov2h_slam_epi_stats.  Returns the number of removed ids, or a
// negative ov2_status.  The fields EpiStats gained with the mono do_optimize branch are read through ov2h_epi_opt_stats.
int ov2h_epipolar_filtering(void *p, void *ctx, int kf_prev, int kf_cur, int nransac_iter, float fransac_err,
                            unsigned long long seed, int cap, int *removed, double *stats)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kf_cur);
    if (!f || !m->map->getKeyframe(kf_prev)) return (int)OV2_ERR_INVALID;
    std::vector<int> before;
    for (const auto &kv : f->mapkps_) before.push_back(kv.first);
    std::sort(before.begin(), before.end());
    SlamParams &S = *m->st;
    S.nransac_iter_ = nransac_iter; S.fransac_err_ = fransac_err; S.bdo_random_ = false; S.epi_seed_ = (uint64_t)seed;
    const int own = f->kfid_;
    f->kfid_ = kf_prev;
    m->map->pcurframe_ = f;
    VisualFrontEnd fe((ov2_ctx *)ctx, m->st, f, m->map, nullptr);
    EpiStats es;
    const ov2_status s = fe.epipolar2d2dFiltering(&es);
    f->kfid_ = own;
    m->last_epi = es;
    if (stats) { stats[0] = es.status; stats[1] = es.pairs; stats[2] = es.removed; stats[3] = es.gate_removed; }
    if (s != OV2_OK) return (int)s;
    int n = 0;
    for (const int id : before)
        if (!f->mapkps_.count(id)) { if (n < cap) removed[n] = id; ++n; }
    return n;
}

// the do_optimize fields of the EpiStats of the last ov2h_epipolar_filtering / ov2h_check_ready_for_init on this map:
// out[3] = do_optimize, the refinement's status, its LM iterations
void ov2h_epi_opt_stats(void *p, int *out)
{
    const EpiStats &e = ((HostMap *)p)->last_epi;
    out[0] = e.do_optimize; out[1] = e.refine_status; out[2] = e.refine_iters;
}

// VisualFrontEnd::checkReadyForInit (:855-984) with keyframe kf_cur taken as the current frame and kf_prev as its keyframe;
// nransac_iter / fransac_err / finit_parallax as the YAML keys, bdo_random off (seed used as is).  removed[cap]: the ids the
// stage removed from kf_cur, ascending (count in *n_removed); stats[4] as ov2h_epipolar_filtering (status: the 5-point call's
// bool).  Returns the reference's bool (0 / 1) or a negative ov2_status.
int ov2h_check_ready_for_init(void *p, void *ctx, int kf_prev, int kf_cur, int nransac_iter, float fransac_err,
                              float finit_parallax, unsigned long long seed, int cap, int *removed, int *n_removed, double *stats)
{
    HostMap *m = (HostMap *)p;
    auto f = m->map->getKeyframe(kf_cur);
    if (!f || !m->map->getKeyframe(kf_prev)) return (int)OV2_ERR_INVALID;
    std::vector<int> before;
    for (const auto &kv : f->mapkps_) before.push_back(kv.first);
    std::sort(before.begin(), before.end());
    SlamParams &S = *m->st;
    S.nransac_iter_ = nransac_iter; S.fransac_err_ = fransac_err; S.finit_parallax_ = finit_parallax;
    S.bdo_random_ = false; S.epi_seed_ = (uint64_t)seed;
    const int own = f->kfid_;
    f->kfid_ = kf_prev;
    m->map->pcurframe_ = f;
    VisualFrontEnd fe((ov2_ctx *)ctx, m->st, f, m->map, nullptr);
    EpiStats es;
    ov2_status s = OV2_OK;
    const bool ready = fe.checkReadyForInit(&es, &s);
    f->kfid_ = own;
    m->last_epi = es;
    if (stats) { stats[0] = es.status; stats[1] = es.pairs; stats[2] = es.removed; stats[3] = es.gate_removed; }
    if (s != OV2_OK) return (int)s;
    int n = 0;
    for (const int id : before)
        if (!f->mapkps_.count(id)) { if (n < cap) removed[n] = id; ++n; }
    if (n_removed) *n_removed = n;
    return ready ? 1 : 0;
}

// MultiViewGeometry::compute5ptEssentialMatrixOpt (the reference's call with do_optimize = true): returns its bool (0 / 1) or
// a negative ov2_status; R9 / t3 / outidx / n_out as ov2h_compute5pt, refine[2] = the refinement's status and LM iterations
int ov2h_compute5pt_opt(void *ctx, int n, const double *bvs1, const double *bvs2, int nmaxiter, float errth, float fx, float fy,
                        unsigned long long seed, double *R9, double *t3, int *outidx, int *n_out, int *refine)
{
    std::vector<Vec3> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[i] = Vec3{bvs1[3 * i], bvs1[3 * i + 1], bvs1[3 * i + 2]};
        b[i] = Vec3{bvs2[3 * i], bvs2[3 * i + 1], bvs2[3 * i + 2]};
    }
    std::vector<int> out;
    ov2_status st = OV2_OK;
    const bool ok = MultiViewGeometry::compute5ptEssentialMatrixOpt((ov2_ctx *)ctx, a, b, nmaxiter, errth, seed, fx, fy, R9, t3,
                                                                    out, &st, refine);
    if (st != OV2_OK) return (int)st;
    for (size_t i = 0; i < out.size(); ++i) outidx[i] = out[i];
    *n_out = (int)out.size();
    return ok ? 1 : 0;
}

// MultiViewGeometry::compute5ptEssentialMatrix (src/multi_view_geometry.cpp:596-697) with the reference's arguments:
// returns its bool (0 / 1) or a negative ov2_status; R9 / t3 = [R12 | t12] when it returns 1, outidx[n] the voutliersidx
// (count in *n_out)
int ov2h_compute5pt(void *ctx, int n, const double *bvs1, const double *bvs2, int nmaxiter, float errth, int boptimize,
                    float fx, float fy, unsigned long long seed, double *R9, double *t3, int *outidx, int *n_out)
{
    std::vector<Vec3> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[i] = Vec3{bvs1[3 * i], bvs1[3 * i + 1], bvs1[3 * i + 2]};
        b[i] = Vec3{bvs2[3 * i], bvs2[3 * i + 1], bvs2[3 * i + 2]};
    }
    std::vector<int> out;
    ov2_status st = OV2_OK;
    const bool ok = MultiViewGeometry::compute5ptEssentialMatrix((ov2_ctx *)ctx, a, b, nmaxiter, errth, boptimize != 0, seed, fx,
                                                                 fy, R9, t3, out, &st);
    if (st != OV2_OK) return (int)st;
    for (size_t i = 0; i < out.size(); ++i) outidx[i] = out[i];
    *n_out = (int)out.size();
    return ok ? 1 : 0;
}

// MultiViewGeometry::p3pRansac (src/multi_view_geometry.cpp:144-163) with the reference's arguments: returns its bool (0 / 1)
// or a negative ov2_status; Twc7 is updated when it returns 1, outidx[n] the voutliersidx (count in *n_out)
int ov2h_p3p_ransac(void *ctx, int n, const double *bvs, const double *wpts, int nmaxiter, float errth, int boptimize,
                    int bdorandom, float fx, float fy, int use_lmeds, unsigned long long seed, double *Twc7, int *outidx, int *n_out)
{
    std::vector<Vec3> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[i] = Vec3{bvs[3 * i], bvs[3 * i + 1], bvs[3 * i + 2]};
        b[i] = Vec3{wpts[3 * i], wpts[3 * i + 1], wpts[3 * i + 2]};
    }
    SE3 T;
    for (int i = 0; i < 7; ++i) T.v[i] = Twc7[i];
    std::vector<int> out;
    ov2_status st = OV2_OK;
    const bool ok = MultiViewGeometry::p3pRansac((ov2_ctx *)ctx, a, b, nmaxiter, errth, boptimize != 0, bdorandom != 0, fx, fy, T, out,
                                                 use_lmeds != 0, seed, &st);
    if (st != OV2_OK) return (int)st;
    for (int i = 0; i < 7; ++i) Twc7[i] = T.v[i];
    for (size_t i = 0; i < out.size(); ++i) outidx[i] = out[i];
    *n_out = (int)out.size();
    return ok ? 1 : 0;
}

int ov2h_get_pose(void *p, int kfid, double *Twc7)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    for (int i = 0; i < 7; ++i) Twc7[i] = f->Twc_.v[i];
    return 0;
}

int ov2h_get_landmark(void *p, int lmid, double *xyz, int *n_obs)
{
    auto lm = ((HostMap *)p)->map->getMapPoint(lmid);
    if (!lm) return -1;
    xyz[0] = lm->ptxyz_.x; xyz[1] = lm->ptxyz_.y; xyz[2] = lm->ptxyz_.z;
    if (n_obs) *n_obs = (int)lm->set_kfids_.size();
    return 0;
}

int ov2h_count_keypoints(void *p, int kfid, int *nbkps, int *nb3d, int *nbstereo)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    *nbkps = (int)f->nbkps_; *nb3d = (int)f->nb3dkps_; *nbstereo = (int)f->nb_stereo_kps_;
    return 0;
}

// out[5]: nbkps_, nb2dkps_, nb3dkps_, nb_stereo_kps_, noccupcells_ of keyframe kfid
int ov2h_frame_counters(void *p, int kfid, int *out)
{
    auto f = ((HostMap *)p)->map->getKeyframe(kfid);
    if (!f) return -1;
    out[0] = (int)f->nbkps_; out[1] = (int)f->nb2dkps_; out[2] = (int)f->nb3dkps_; out[3] = (int)f->nb_stereo_kps_;
    out[4] = (int)f->noccupcells_;
    return 0;
}

// MapPoint::isobs_ of landmark lmid (1 / 0), -1 if the map does not hold it
int ov2h_landmark_isobs(void *p, int lmid)
{
    auto lm = ((HostMap *)p)->map->getMapPoint(lmid);
    return lm ? (lm->isobs_ ? 1 : 0) : -1;
}

// ---------------------------------------------------------------------------------------------------------------
// ov2::SlamManager (ov2_slam.hpp): one stereo frame per call through visualTracking and, on keyframes, Mapper::run +
// Estimator::applyLocalBA -- the closed loop in C++.  policy = {kf_every, ba_window, ba_fixed, compose_motion, midpoint_stereo,
// pose_from_kf} (all zero = the reference's own heuristics); rect != 0: rectified rig (bdo_stereo_rect_).
void *ov2h_slam_create(void *ctx, const double *K4, double baseline, int w, int h, int cell, int rect, const int *policy, int use_device_map)
{
    auto st = std::make_shared<SlamParams>();
    st->stereo_ = true; st->mono_ = false; st->bdo_stereo_rect_ = rect != 0;
    st->nmaxdist_ = cell;
    st->nbmaxkps_ = (int)(std::ceil((float)w / cell) * std::ceil((float)h / cell));   // src/slam_params.cpp:107-110
    auto cl = std::make_shared<CameraCalibration>(), cr = std::make_shared<CameraCalibration>();
    cl->fx_ = cr->fx_ = K4[0]; cl->fy_ = cr->fy_ = K4[1]; cl->cx_ = cr->cx_ = K4[2]; cl->cy_ = cr->cy_ = K4[3];
    cl->img_w_ = cr->img_w_ = w; cl->img_h_ = cr->img_h_ = h;
    cr->Tc0ci_.v = {baseline, 0, 0, 0, 0, 0, 1};
    LoopPolicy pol;
    if (policy) {
        pol.kf_every = policy[0]; pol.ba_window = policy[1]; pol.ba_fixed = policy[2]; pol.compose_motion = policy[3] != 0;
        pol.midpoint_stereo = policy[4] != 0; pol.pose_from_kf = policy[5] != 0;
    }
    SlamManager *S = new SlamManager((ov2_ctx *)ctx, st, cl, cr, pol);
    if (use_device_map && S->pmap_->attachDevice((ov2_ctx *)ctx, 64, 4096, 16384) != OV2_OK) { delete S; return nullptr; }
    return S;
}

int ov2h_slam_add_stereo(void *p, double time, const uint8_t *left, const uint8_t *right, int w, int h)
{
    return (int)((SlamManager *)p)->addNewStereoImages(time, left, right, w, h, w);
}

void ov2h_slam_pose(void *p, double *Twc7)
{
    const SE3 T = ((SlamManager *)p)->pose();
    for (int i = 0; i < 7; ++i) Twc7[i] = T.v[i];
}

// out[16]: frame, keypoints, 3D keypoints, keyframe?, new keypoints, stereo keypoints, 3D landmarks, BA ran?, residual blocks,
// robust iterations, L2 iterations, outliers, cost before, cost after, keyframes so far, landmarks so far
void ov2h_slam_stats(void *p, double *out)
{
    SlamManager *S = (SlamManager *)p;
    const SlamStats &s = S->last_;
    const double v[16] = {(double)s.frame, (double)s.tracked, (double)s.n3d, (double)s.is_kf, (double)s.n_new, (double)s.n_stereo,
                          (double)s.n_lm3d, (double)s.ba_done, (double)s.ba_res, (double)s.ba_it_robust, (double)s.ba_it_l2,
                          (double)s.ba_outliers, s.ba_cost0, s.ba_cost1, (double)S->pmap_->map_pkfs_.size(), (double)S->pmap_->map_plms_.size()};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
}

// ids + world points of the 3D landmarks (capacity cap); returns the count
int ov2h_slam_landmarks(void *p, int cap, int *lmid, double *xyz)
{
    SlamManager *S = (SlamManager *)p;
    std::vector<int> ids;
    for (const auto &kv : S->pmap_->map_plms_) if (kv.second->is3d_) ids.push_back(kv.first);
    std::sort(ids.begin(), ids.end());
    int n = 0;
    for (int id : ids) {
        if (n < cap) { const Vec3 q = S->pmap_->getMapPoint(id)->getPoint(); lmid[n] = id; xyz[3 * n] = q.x; xyz[3 * n + 1] = q.y; xyz[3 * n + 2] = q.z; }
        ++n;
    }
    return n;
}

void ov2h_slam_destroy(void *p) { delete (SlamManager *)p; }

// keyframe descriptors + Mapper::matchingToLocalMap: pattern = the 256 x 4 int8 BRIEF test table (NULL keeps the current one)
void ov2h_slam_set_brief(void *p, const int8_t *pattern, int use_brief, int track_localmap, float fmax_desc_dist, float fmax_proj_pxdist)
{
    SlamManager *S = (SlamManager *)p;
    if (pattern) S->setBriefPattern(pattern);
    S->pslamstate_->use_brief_ = use_brief != 0;
    S->pslamstate_->bdo_track_localmap_ = track_localmap != 0;
    if (fmax_desc_dist > 0.f) S->pslamstate_->fmax_desc_dist_ = fmax_desc_dist;
    if (fmax_proj_pxdist > 0.f) S->pslamstate_->fmax_proj_pxdist_ = fmax_proj_pxdist;
}

// VisualFrontEnd::epipolar2d2dFiltering in trackMono (YAML doepipolar, nransac_iter, fransac_err, bdo_random) + the sampler's
// base seed (bdo_random: mixed with the frame id; otherwise used as is on every frame)
void ov2h_slam_set_epipolar(void *p, int on, int nransac_iter, float fransac_err, int bdo_random, unsigned long long seed)
{
    SlamParams &S = *((SlamManager *)p)->pslamstate_;
    S.doepipolar_ = on != 0;
    S.nransac_iter_ = nransac_iter;
    S.fransac_err_ = fransac_err;
    S.bdo_random_ = bdo_random != 0;
    S.epi_seed_ = (uint64_t)seed;
}

// out[4] of the last frame: RANSAC status (-1 = returned before it), pairs, outliers removed, 2D keypoints removed by the gate
void ov2h_slam_epi_stats(void *p, double *out)
{
    const EpiStats &e = ((SlamManager *)p)->last_epi_;
    out[0] = e.status; out[1] = e.pairs; out[2] = e.removed; out[3] = e.gate_removed;
}

// dop3p of the YAML: computePose runs the P3P-LMedS bootstrap on every frame (nransac_iter, fransac_err, bdo_random and the
// base seed are those of ov2h_slam_set_epipolar)
void ov2h_slam_set_p3p(void *p, int dop3p) { ((SlamManager *)p)->pslamstate_->dop3p_ = dop3p != 0; }

// out[5] of the last frame: the P3P branch ran, p3pRansac's return, correspondences in, observations removed, resetFrame()
void ov2h_slam_p3p_stats(void *p, double *out)
{
    const P3pStats &e = ((SlamManager *)p)->last_p3p_;
    out[0] = e.ran; out[1] = e.status; out[2] = e.points; out[3] = e.removed; out[4] = e.reset;
}

// Mapper::triangulateTemporal in Mapper::run (src/mapper.cpp:107-126); off by default, see SlamParams::do_temporal_
void ov2h_slam_set_temporal(void *p, int on) { ((SlamManager *)p)->pslamstate_->do_temporal_ = on != 0; }

// out[5] of the last keyframe: the stage ran, 2D keypoints offered, candidates, good, observations removed
void ov2h_slam_temporal_stats(void *p, double *out)
{
    const TemporalStats &t = ((SlamManager *)p)->last_temporal_;
    out[0] = t.ran; out[1] = t.n_kps; out[2] = t.n_candidates; out[3] = t.n_good; out[4] = t.n_removed;
}

// out[3] of the last frame (keyframes only): keypoints described, local map points offered to matchToMap, merges
// kf_filtering_ratio of the YAML (Estimator::mapFiltering after every local BA); 1 = off, the default
void ov2h_slam_set_kf_filtering(void *p, float ratio) { ((SlamManager *)p)->pslamstate_->fkf_filtering_ratio_ = ratio; }

// what Estimator::mapFiltering did on the last keyframe: ran, candidates, removed, removed by the nb3dkps_ rule, is3d_ cleared,
// then up to 11 removed kfids in order (-1 beyond)
void ov2h_slam_filter_stats(void *p, double *out)
{
    const FilterStats &f = ((SlamManager *)p)->pestimator_->last_filter_;
    out[0] = f.ran; out[1] = f.n_candidates; out[2] = (double)f.removed.size(); out[3] = f.n_few3d; out[4] = (double)f.unset3d.size();
    for (int i = 0; i < 11; ++i) out[5 + i] = i < (int)f.removed.size() ? f.removed[i] : -1;
}

void ov2h_slam_kf_stats(void *p, double *out)
{
    const SlamStats &s = ((SlamManager *)p)->last_;
    out[0] = s.n_described; out[1] = s.n_local; out[2] = s.n_matched;
}

void *ov2h_slam_device_handle(void *p) { return ((SlamManager *)p)->pmap_->dev_; }
int ov2h_slam_flush_device(void *p) { return (int)((SlamManager *)p)->pmap_->flushDevice(); }

// Invariants of the host map after any sequence of frames.  out[6]: keypoints of keyframes whose map point is missing,
// keypoints whose map point does not list the keyframe, observers a map point lists that do not hold it (or are gone),
// covisibility entries that differ from the count of co-observed map points, 3D map points without a descriptor although
// use_brief_ is on, map points with descriptors from keyframes that do not observe them.  returns their sum
int ov2h_slam_check_map(void *p, int *out)
{
    SlamManager *S = (SlamManager *)p;
    MapManager &M = *S->pmap_;
    int v[6] = {0, 0, 0, 0, 0, 0};
    for (const auto &kf : M.map_pkfs_) {
        std::map<int, int> cov;
        for (const auto &kv : kf.second->mapkps_) {
            auto plm = M.getMapPoint(kv.first);
            if (!plm) { ++v[0]; continue; }
            if (!plm->set_kfids_.count(kf.first)) ++v[1];
            for (int o : plm->set_kfids_) if (o != kf.first && M.getKeyframe(o)) cov[o]++;
        }
        for (const auto &c : cov) { auto it = kf.second->map_covkfs_.find(c.first); if (it == kf.second->map_covkfs_.end() || it->second != c.second) ++v[3]; }
        for (const auto &c : kf.second->map_covkfs_) if (!cov.count(c.first) && M.getKeyframe(c.first)) ++v[3];
    }
    for (const auto &lm : M.map_plms_) {
        for (int kfid : lm.second->set_kfids_) {
            auto pkf = M.getKeyframe(kfid);
            if (!pkf || !pkf->mapkps_.count(lm.first)) ++v[2];
        }
        if (S->pslamstate_->use_brief_ && lm.second->is3d_ && !lm.second->has_desc_) ++v[4];
        for (const auto &d : lm.second->map_kf_desc_) if (!lm.second->set_kfids_.count(d.first)) ++v[5];
    }
    int tot = 0;
    for (int i = 0; i < 6; ++i) { if (out) out[i] = v[i]; tot += v[i]; }
    return tot;
}

// the host map as flat arrays (capacity caps; counts come back in n[3] = keyframes, landmarks, observations):
// keyframes (id, Twc), landmarks (id, xyz, state bits: 1 alive | 2 is3d | 4 isobs), observations (kfid, lmid, stereo)
void ov2h_slam_export_map(void *p, int cap_kf, int cap_lm, int cap_obs, int *n, int *kf_id, double *kf_pose, int *lm_id, double *lm_xyz,
                          uint8_t *lm_state, int *obs_kf, int *obs_lm, uint8_t *obs_stereo)
{
    MapManager &M = *((SlamManager *)p)->pmap_;
    int nk = 0, nl = 0, no = 0;
    std::map<int, std::shared_ptr<Frame>> kfs(M.map_pkfs_.begin(), M.map_pkfs_.end());
    for (const auto &kf : kfs) {
        if (nk < cap_kf) { kf_id[nk] = kf.first; const SE3 T = kf.second->getTwc(); for (int i = 0; i < 7; ++i) kf_pose[7 * nk + i] = T.v[i]; }
        ++nk;
        std::map<int, Keypoint> kps(kf.second->mapkps_.begin(), kf.second->mapkps_.end());
        for (const auto &kv : kps) {
            if (no < cap_obs) { obs_kf[no] = kf.first; obs_lm[no] = kv.first; obs_stereo[no] = kv.second.is_stereo_ ? 1 : 0; }
            ++no;
        }
    }
    std::map<int, std::shared_ptr<MapPoint>> lms(M.map_plms_.begin(), M.map_plms_.end());
    for (const auto &lm : lms) {
        if (nl < cap_lm) {
            lm_id[nl] = lm.first; const Vec3 q = lm.second->getPoint(); lm_xyz[3 * nl] = q.x; lm_xyz[3 * nl + 1] = q.y; lm_xyz[3 * nl + 2] = q.z;
            lm_state[nl] = (uint8_t)(1 | (lm.second->is3d_ ? 2 : 0) | (lm.second->isobs_ ? 4 : 0));
        }
        ++nl;
    }
    n[0] = nk; n[1] = nl; n[2] = no;
}

// ---- MapPoint descriptor bookkeeping alone (tests: against a restatement of src/map_point.cpp:106-211) ----
void *ov2h_mp_new(int lmid, int kfid, const uint8_t *desc)
{
    if (!desc) return new MapPoint(lmid, kfid, true);
    Desc d; std::copy(desc, desc + 32, d.begin());
    return new MapPoint(lmid, kfid, d, true);
}
void ov2h_mp_add_obs(void *p, int kfid) { ((MapPoint *)p)->addKfObs(kfid); }
void ov2h_mp_add_desc(void *p, int kfid, const uint8_t *desc) { Desc d; std::copy(desc, desc + 32, d.begin()); ((MapPoint *)p)->addDesc(kfid, d); }
void ov2h_mp_remove_obs(void *p, int kfid) { ((MapPoint *)p)->removeKfObs(kfid); }
// out_i[4] = has_desc, anchor kfid, observers, descriptors; desc[32] = the representative one; per descriptor (cap): kfid + summed distance
int ov2h_mp_state(void *p, int *out_i, uint8_t *desc, int cap, int *kfids, float *dists)
{
    MapPoint &m = *(MapPoint *)p;
    out_i[0] = m.has_desc_ ? 1 : 0; out_i[1] = m.kfid_; out_i[2] = (int)m.set_kfids_.size(); out_i[3] = (int)m.map_kf_desc_.size();
    std::copy(m.desc_.begin(), m.desc_.end(), desc);
    std::map<int, float> d(m.map_desc_dist_.begin(), m.map_desc_dist_.end());
    int n = 0;
    for (const auto &kv : d) { if (n < cap) { kfids[n] = kv.first; dists[n] = kv.second; } ++n; }
    return n;
}
void ov2h_mp_free(void *p) { delete (MapPoint *)p; }

// ---------------------------------------------------------------------------------------------------------------
// Estimator threads of `nseq` SLAM instances (reference src/estimator.cpp:32-98 run(): wait for a keyframe ->
// applyLocalBA -> next), served by ONE native thread with its own HIP context: it takes every sequence that has a
// keyframe pending and solves their windows in one ov2_ba_solve_batch call (at most max_batch windows per call).  A
// keyframe that arrives while its sequence still has one pending replaces it (the reference keeps only the newest,
// src/estimator.cpp:185-210).  Every job solves a fresh copy of the window it was created with.  Native so that it runs
// beside a Python front-end loop without sharing the interpreter lock.
struct BaWorkerNative {
    ov2_ctx *ctx = nullptr;
    std::vector<double> pose0, lm0, lm_auv, res_uv, res_sigma;
    std::vector<uint8_t> pose_const, res_type;
    std::vector<int32_t> lm_anchor, res_pose, res_lm;
    ov2_ba_problem P{};
    ov2_ba_options opt{};
    int max_batch = 64;
    std::vector<uint8_t> pending;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;
    bool stop = false, counting = false;
    long long solves = 0, iters = 0, dropped = 0, submitted = 0, batches = 0;
    double busy_s = 0.0;
    int last_status = 0;

    // device-resident windows (ov2_ba_solve_batch_dev): the window's arrays are uploaded once, every job solves its own
    // device copy of the state -- what a device-side producer of the problems (the map mirror) hands over
    bool device_resident = false;
    ov2_ba_problem Pd{};                       // P with device pointers
    std::vector<void *> pose_d, lm_d, owned_d;

    bool dev_setup()
    {
        auto up = [&](const void *h, size_t bytes) -> void * {
            if (!h || !bytes) return nullptr;
            void *d = nullptr;
            if (ov2_dev_alloc(ctx, bytes, &d) != OV2_OK) return nullptr;
            owned_d.push_back(d);
            if (ov2_memcpy_h2d(ctx, d, h, bytes) != OV2_OK) return nullptr;
            return d;
        };
        const size_t e = P.inv_depth ? 1 : 3, np = (size_t)P.n_pose, nl = (size_t)P.n_lm, nr = (size_t)P.n_res;
        Pd = P;
        Pd.pose_const = (const uint8_t *)up(P.pose_const, np);
        Pd.lm_anchor_pose = (const int32_t *)up(P.lm_anchor_pose, nl * 4);
        Pd.lm_anchor_uv = (const double *)up(P.lm_anchor_uv, 2 * nl * 8);
        Pd.res_type = (const uint8_t *)up(P.res_type, nr);
        Pd.res_pose = (const int32_t *)up(P.res_pose, nr * 4);
        Pd.res_lm = (const int32_t *)up(P.res_lm, nr * 4);
        Pd.res_uv = (const double *)up(P.res_uv, 2 * nr * 8);
        Pd.res_sigma = (const double *)up(P.res_sigma, nr * 8);
        (void)e;
        return (Pd.res_uv || !nr) && (Pd.pose_const || !np) && (Pd.res_type || !nr);
    }

    // a fresh copy of the window per job: the states of all jobs of a batch live in two contiguous device buffers that
    // are re-filled from pre-replicated templates with two copies per batch (one copy per job and array was 128 small
    // transfers in front of every batch of 64)
    void *tmpl_pose_d = nullptr, *tmpl_lm_d = nullptr, *state_pose_d = nullptr, *state_lm_d = nullptr;
    size_t state_cap = 0;

    bool dev_job_state(size_t nb)
    {
        const size_t e = P.inv_depth ? 1 : 3, pb = 7 * (size_t)P.n_pose * 8, lb = e * (size_t)P.n_lm * 8;
        if (nb > state_cap) {
            const size_t cap = std::max<size_t>(nb, (size_t)max_batch);
            std::vector<double> rp((size_t)7 * P.n_pose * cap), rl(e * (size_t)P.n_lm * cap);
            for (size_t k = 0; k < cap; ++k) {
                std::copy(pose0.begin(), pose0.end(), rp.begin() + k * pose0.size());
                std::copy(lm0.begin(), lm0.end(), rl.begin() + k * lm0.size());
            }
            void *bufs[4] = {nullptr, nullptr, nullptr, nullptr};
            const size_t bytes[4] = {pb * cap, lb * cap, pb * cap, lb * cap};
            for (int i = 0; i < 4; ++i) {
                if (ov2_dev_alloc(ctx, bytes[i] ? bytes[i] : 8, &bufs[i]) != OV2_OK) return false;
                owned_d.push_back(bufs[i]);
            }
            if (pb && ov2_memcpy_h2d(ctx, bufs[0], rp.data(), pb * cap) != OV2_OK) return false;
            if (lb && ov2_memcpy_h2d(ctx, bufs[1], rl.data(), lb * cap) != OV2_OK) return false;
            tmpl_pose_d = bufs[0]; tmpl_lm_d = bufs[1]; state_pose_d = bufs[2]; state_lm_d = bufs[3];
            state_cap = cap;
            pose_d.assign(cap, nullptr); lm_d.assign(cap, nullptr);
            for (size_t k = 0; k < cap; ++k) { pose_d[k] = (char *)state_pose_d + k * pb; lm_d[k] = (char *)state_lm_d + k * lb; }
        }
        if (pb && ov2_memcpy_d2d(ctx, state_pose_d, tmpl_pose_d, pb * nb) != OV2_OK) return false;   // on the solver's stream
        if (lb && ov2_memcpy_d2d(ctx, state_lm_d, tmpl_lm_d, lb * nb) != OV2_OK) return false;
        return true;
    }

    void loop()
    {
        size_t rr = 0;
        bool dev_ready = false, dev_failed = false, use_dev = false;
        std::vector<int> jobs;
        std::vector<std::vector<double>> poses, lms;   // per job: the window's own state (solved in place)
        std::vector<ov2_ba_problem> Ps;
        std::vector<ov2_ba_result> Rs;
        for (;;) {
            jobs.clear();
            bool counted = false;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (stop) return;
                    for (size_t k = 0; k < pending.size() && (int)jobs.size() < max_batch; ++k) {
                        const size_t b = (rr + k) % pending.size();
                        if (pending[b]) { pending[b] = 0; jobs.push_back((int)b); }
                    }
                    if (!jobs.empty()) { rr = ((size_t)jobs.back() + 1) % pending.size(); break; }
                    cv.wait_for(lk, std::chrono::milliseconds(2));
                }
                counted = counting;   // a batch counts only if it started inside the counted region
                use_dev = device_resident;   // latched under the mutex ov2h_ba_worker_set_device_resident takes
            }
            const size_t nb = jobs.size();
            if (poses.size() < nb) { poses.resize(nb); lms.resize(nb); }
            Ps.assign(nb, P);
            Rs.resize(nb);
            for (size_t k = 0; k < nb; ++k) {
                if (!use_dev) {
                    poses[k] = pose0; lms[k] = lm0;
                    Ps[k].pose = poses[k].data(); Ps[k].lm = lms[k].data();
                }
                std::memset(&Rs[k], 0, sizeof(ov2_ba_result));
            }
            if (use_dev && !dev_ready && !dev_failed) { dev_ready = dev_setup(); dev_failed = !dev_ready; }   // a failed upload is not retried
            const auto t0 = std::chrono::steady_clock::now();
            ov2_status s;
            if (use_dev) {
                s = OV2_ERR_NOMEM;
                if (dev_ready && dev_job_state(nb)) {
                    Ps.assign(nb, Pd);
                    for (size_t k = 0; k < nb; ++k) { Ps[k].pose = (double *)pose_d[k]; Ps[k].lm = (double *)lm_d[k]; }
                    s = ov2_ba_solve_batch_dev(ctx, (int)nb, Ps.data(), &opt, Rs.data());
                }
            } else {
                s = ov2_ba_solve_batch(ctx, (int)nb, Ps.data(), &opt, Rs.data());
            }
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::lock_guard<std::mutex> lk(mu);
            if (last_status == 0) last_status = s;   // sticky: a later good batch must not hide a failed one from stats()
            if (counted && counting && s == OV2_OK) {   // ... and finished inside it
                ++batches;
                for (size_t k = 0; k < nb; ++k) {
                    ++solves;
                    const int it = Rs[k].n_log - 1 - (Rs[k].l2_done ? 1 : 0);   // the log holds one iteration-0 record per solve
                    iters += it > 0 ? it : 0;
                }
                busy_s += dt;
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// The same Estimator threads with the WHOLE of Optimizer::localBA per keyframe job, on device-resident maps: every
// sequence owns an ov2_map (its own keyframes / landmarks / observations, its own window size and outlier rate); a job is
//     [the mapper's edits: here the map is rewound to its saved state, ov2_map_restore_state_batch]
//     set-up   ov2_map_local_ba_setup_batch    src/optimizer.cpp:43-430   (one synchronisation for all pending maps)
//     solve    ov2_ba_solve_batch_dev          :439-735                   (on the flat problems the set-up left in HBM)
//     update   ov2_map_local_ba_update_batch   :741-882                   (on the tables, asynchronous)
// and a batch ends with one synchronisation of the worker's context, so that the counted time closes over all three stages.
// The context and the maps are created by the caller (on that context) and belong to this thread until it is destroyed.
struct BaPipelineNative {
    ov2_ctx *ctx = nullptr;
    std::vector<ov2_map *> maps;
    std::vector<int32_t> newkf;
    std::vector<double> calib_l;   // nseq x 4
    ov2_ba_problem proto{};
    ov2_ba_options opt{};
    int inv_depth = 1, max_batch = 64;
    std::vector<uint8_t> pending;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;
    bool stop = false, counting = false;
    long long solves = 0, iters = 0, dropped = 0, submitted = 0, batches = 0, slowest_sum = 0, res_blocks = 0, aborted = 0, iter_blocks = 0;
    long long hist_robust[8] = {0}, hist_l2[16] = {0};
    double busy_s = 0.0, t_setup = 0.0, t_solve = 0.0, t_update = 0.0;
    int last_status = 0;

    void loop()
    {
        size_t rr = 0;
        std::vector<int> jobs;
        std::vector<ov2_map *> M;
        std::vector<int32_t> nk;
        std::vector<double> K;
        std::vector<ov2_local_ba_setup> V;
        std::vector<ov2_ba_problem> Ps;
        std::vector<ov2_ba_result> Rs;
        std::vector<const uint8_t *> outl;
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double>(b - a).count();
        };
        for (;;) {
            jobs.clear();
            bool counted = false;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (stop) return;
                    for (size_t k = 0; k < pending.size() && (int)jobs.size() < max_batch; ++k) {
                        const size_t b = (rr + k) % pending.size();
                        if (pending[b]) { pending[b] = 0; jobs.push_back((int)b); }
                    }
                    if (!jobs.empty()) { rr = ((size_t)jobs.back() + 1) % pending.size(); break; }
                    cv.wait_for(lk, std::chrono::milliseconds(2));
                }
                counted = counting;   // a batch counts only if it started inside the counted region
            }
            const int nb = (int)jobs.size();
            M.resize(nb); nk.resize(nb); K.resize(4 * (size_t)nb); V.resize(nb); Ps.resize(nb); Rs.resize(nb); outl.resize(nb);
            for (int k = 0; k < nb; ++k) {
                M[k] = maps[jobs[k]]; nk[k] = newkf[jobs[k]];
                for (int q = 0; q < 4; ++q) K[4 * (size_t)k + q] = calib_l[4 * (size_t)jobs[k] + q];
            }
            const auto t0 = now();
            ov2_status s = ov2_map_restore_state_batch(ctx, nb, M.data());
            if (s == OV2_OK) s = ov2_map_local_ba_setup_batch(ctx, nb, M.data(), nk.data(), 25, 1, inv_depth, K.data(), V.data());
            const auto t1 = now();
            long long blocks = 0, nab = 0;
            if (s == OV2_OK) {
                for (int k = 0; k < nb; ++k) {
                    const ov2_local_ba_setup &v = V[k];
                    ov2_ba_problem &P = Ps[k];
                    P = proto;
                    for (int q = 0; q < 4; ++q) P.calib_l[q] = K[4 * (size_t)k + q];
                    P.inv_depth = inv_depth;
                    if (v.aborted) { P.n_pose = P.n_lm = P.n_res = 0; ++nab; }
                    else { P.n_pose = v.n_pose; P.n_lm = v.n_lm; P.n_res = v.n_res; blocks += v.n_res; }
                    P.pose = v.pose; P.pose_const = v.pose_const; P.lm = v.lm; P.lm_anchor_pose = v.lm_anchor_pose; P.lm_anchor_uv = v.lm_anchor_uv;
                    P.res_type = v.res_type; P.res_pose = v.res_pose; P.res_lm = v.res_lm; P.res_uv = v.res_uv; P.res_sigma = v.res_sigma;
                    std::memset(&Rs[k], 0, sizeof(ov2_ba_result));
                    Rs[k].outlier = v.aborted ? nullptr : v.res_outlier;
                    outl[k] = Rs[k].outlier;
                }
                s = ov2_ba_solve_batch_dev(ctx, nb, Ps.data(), &opt, Rs.data());
            }
            const auto t2 = now();
            if (s == OV2_OK) s = ov2_map_local_ba_update_batch(ctx, nb, M.data(), outl.data(), nk.data(), nullptr);
            if (s == OV2_OK) s = ov2_ctx_synchronize(ctx);
            const auto t3 = now();
            std::lock_guard<std::mutex> lk(mu);
            if (last_status == 0) last_status = s;   // sticky: a later good batch must not hide a failed one from stats()
            if (counted && counting && s == OV2_OK) {   // ... and finished inside it
                ++batches;
                int slowest = 0;
                for (int k = 0; k < nb; ++k) {
                    ++solves;
                    const int n1 = Rs[k].n_log_robust > 0 ? Rs[k].n_log_robust - 1 : 0;
                    const int n2 = Rs[k].l2_done ? Rs[k].n_log - Rs[k].n_log_robust - 1 : 0;
                    iters += n1 + (n2 > 0 ? n2 : 0);
                    hist_robust[n1 < 7 ? n1 : 7]++;
                    hist_l2[n2 < 0 ? 0 : (n2 < 15 ? n2 : 15)]++;
                    slowest = std::max(slowest, n1 + (n2 > 0 ? n2 : 0));
                    iter_blocks += (long long)(n1 + (n2 > 0 ? n2 : 0)) * Ps[k].n_res;
                }
                slowest_sum += slowest; res_blocks += blocks; aborted += nab;
                busy_s += sec(t0, t3); t_setup += sec(t0, t1); t_solve += sec(t1, t2); t_update += sec(t2, t3);
            }
        }
    }
};

void *ov2h_ba_pipeline_create(void *ctx, int nseq, void *const *maps, const int *newkf, const double *calib_l, const ov2_ba_problem *proto,
                              float robust_mono_th, int inv_depth, int max_batch)
{
    if (!ctx || nseq <= 0 || !maps || !newkf || !calib_l || !proto) return nullptr;
    BaPipelineNative *w = new BaPipelineNative();
    w->ctx = (ov2_ctx *)ctx;
    w->maps.assign((ov2_map *const *)maps, (ov2_map *const *)maps + nseq);
    w->newkf.assign(newkf, newkf + nseq);
    w->calib_l.assign(calib_l, calib_l + 4 * (size_t)nseq);
    w->proto = *proto;   // calibrations + extrinsic; the array pointers are replaced per job
    w->inv_depth = inv_depth ? 1 : 0;
    w->max_batch = max_batch > 0 ? max_batch : 1;
    ov2_ba_default_options(&w->opt, robust_mono_th);
    w->pending.assign((size_t)nseq, 0);
    w->th = std::thread([w] { w->loop(); });
    return w;
}

void ov2h_ba_pipeline_submit_all(void *p)
{
    BaPipelineNative *w = (BaPipelineNative *)p;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        for (auto &f : w->pending) {
            if (f && w->counting) ++w->dropped;
            f = 1;
            if (w->counting) ++w->submitted;
        }
    }
    w->cv.notify_one();
}

void ov2h_ba_pipeline_set_counting(void *p, int on)
{
    BaPipelineNative *w = (BaPipelineNative *)p;
    std::lock_guard<std::mutex> lk(w->mu);
    w->counting = on != 0;
}

// out[40]: 0 solves, 1 LM iterations, 2 jobs replaced by a newer keyframe, 3 jobs submitted, 4 busy seconds, 5 last status,
// 6 batches, 7 set-up s, 8 solve s, 9 update s, 10 sum over batches of the slowest window's iterations, 11 residual blocks solved,
// 12 aborted set-ups, 13 sum over windows of LM iterations x residual blocks, 16..23 windows by robust iterations (0..7+), 24..39 windows by L2 iterations (0..15+)
void ov2h_ba_pipeline_stats(void *p, double *out)
{
    BaPipelineNative *w = (BaPipelineNative *)p;
    std::lock_guard<std::mutex> lk(w->mu);
    for (int i = 0; i < 40; ++i) out[i] = 0.0;
    out[0] = (double)w->solves; out[1] = (double)w->iters; out[2] = (double)w->dropped; out[3] = (double)w->submitted;
    out[4] = w->busy_s; out[5] = (double)w->last_status; out[6] = (double)w->batches;
    out[7] = w->t_setup; out[8] = w->t_solve; out[9] = w->t_update; out[10] = (double)w->slowest_sum; out[11] = (double)w->res_blocks;
    out[12] = (double)w->aborted; out[13] = (double)w->iter_blocks;
    for (int i = 0; i < 8; ++i) out[16 + i] = (double)w->hist_robust[i];
    for (int i = 0; i < 16; ++i) out[24 + i] = (double)w->hist_l2[i];
}

// stops the thread; the context and the maps stay with the caller
void ov2h_ba_pipeline_destroy(void *p)
{
    BaPipelineNative *w = (BaPipelineNative *)p;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->stop = true;
    }
    w->cv.notify_all();
    if (w->th.joinable()) w->th.join();
    delete w;
}

void *ov2h_ba_worker_create(int device, const ov2_ba_problem *P, float robust_mono_th, int nseq, int max_batch, int high_priority)
{
    BaWorkerNative *w = new BaWorkerNative();
    w->max_batch = max_batch > 0 ? max_batch : 1;
    if (ov2_ctx_create_ex(device, high_priority ? 1 : 0, &w->ctx) != OV2_OK) { delete w; return nullptr; }
    const int e = P->inv_depth ? 1 : 3;
    w->pose0.assign(P->pose, P->pose + 7 * (size_t)P->n_pose);
    w->lm0.assign(P->lm, P->lm + (size_t)e * P->n_lm);
    w->pose_const.assign(P->pose_const, P->pose_const + P->n_pose);
    if (P->inv_depth) {
        w->lm_anchor.assign(P->lm_anchor_pose, P->lm_anchor_pose + P->n_lm);
        w->lm_auv.assign(P->lm_anchor_uv, P->lm_anchor_uv + 2 * (size_t)P->n_lm);
    }
    w->res_type.assign(P->res_type, P->res_type + P->n_res);
    w->res_pose.assign(P->res_pose, P->res_pose + P->n_res);
    w->res_lm.assign(P->res_lm, P->res_lm + P->n_res);
    w->res_uv.assign(P->res_uv, P->res_uv + 2 * (size_t)P->n_res);
    if (P->res_sigma) w->res_sigma.assign(P->res_sigma, P->res_sigma + P->n_res);
    w->P = *P;
    w->P.pose_const = w->pose_const.data();
    w->P.lm_anchor_pose = P->inv_depth ? w->lm_anchor.data() : nullptr;
    w->P.lm_anchor_uv = P->inv_depth ? w->lm_auv.data() : nullptr;
    w->P.res_type = w->res_type.data(); w->P.res_pose = w->res_pose.data(); w->P.res_lm = w->res_lm.data();
    w->P.res_uv = w->res_uv.data(); w->P.res_sigma = P->res_sigma ? w->res_sigma.data() : nullptr;
    ov2_ba_default_options(&w->opt, robust_mono_th);
    w->pending.assign((size_t)(nseq > 0 ? nseq : 1), 0);
    w->th = std::thread([w] { w->loop(); });
    return w;
}

// before the first submission: the worker keeps its windows in device memory and solves them with ov2_ba_solve_batch_dev
void ov2h_ba_worker_set_device_resident(void *p, int on)
{
    BaWorkerNative *w = (BaWorkerNative *)p;
    std::lock_guard<std::mutex> lk(w->mu);
    w->device_resident = on != 0;
}

// Mapper::run -> Estimator::addNewKf for every sequence of the batch
void ov2h_ba_worker_submit_all(void *p)
{
    BaWorkerNative *w = (BaWorkerNative *)p;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        for (auto &f : w->pending) {
            if (f && w->counting) ++w->dropped;
            f = 1;
            if (w->counting) ++w->submitted;
        }
    }
    w->cv.notify_one();
}

void ov2h_ba_worker_set_counting(void *p, int on)
{
    BaWorkerNative *w = (BaWorkerNative *)p;
    std::lock_guard<std::mutex> lk(w->mu);
    w->counting = on != 0;
}

// out[7] = solves, LM iterations, jobs replaced by a newer keyframe, jobs submitted, busy seconds, last status, batches
void ov2h_ba_worker_stats(void *p, double *out)
{
    BaWorkerNative *w = (BaWorkerNative *)p;
    std::lock_guard<std::mutex> lk(w->mu);
    out[0] = (double)w->solves; out[1] = (double)w->iters; out[2] = (double)w->dropped; out[3] = (double)w->submitted;
    out[4] = w->busy_s; out[5] = (double)w->last_status; out[6] = (double)w->batches;
}

void ov2h_ba_worker_destroy(void *p)
{
    BaWorkerNative *w = (BaWorkerNative *)p;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->stop = true;
    }
    w->cv.notify_all();
    if (w->th.joinable()) w->th.join();
    for (void *d : w->owned_d) ov2_dev_free(w->ctx, d);
    ov2_ctx_destroy(w->ctx);
    delete w;
}


// ---------------------------------------------------------------------------------------------------------------------
// Native per-frame driver of the bench streams: what SlamManager::run's loop does per image for B lock-step sequences
// (preprocessImage -> kltTracking -> ceresPnP; on a keyframe: right pyramid -> stereoMatching -> detector, then the
// keyframe goes to the Estimator workers) over device-resident inputs, enqueued from C++ so that small streams (one
// 308-keypoint sequence) are not bound by the interpreter's ~15 us per ctypes call.  Every pointer is a device pointer
// owned by the caller; nothing is synchronised here.
struct ov2h_feloop_cfg {
    int32_t L, B, n, win, nlvl, use_clahe, tiles_x, tiles_y;
    float clahe_clip, err_th, fb_th, eps;
    int32_t max_iter, detect, det_cell, det_ncur, det_cap, pnp;
    void *const *left, *const *right;                   // L batches of images (ov2_images*)
    const float *const *kps, *const *pri, *const *st_pri;   // per cycle position: n x 2
    const uint8_t *const *has, *const *st_has;
    const int32_t *img_idx;
    float *out_xy; uint8_t *out_st; int32_t *p3p;
    // per-frame pose refinement (one problem per sequence, re-solved from T0 every frame)
    const int32_t *pnp_off; const double *pnp_unpx, *pnp_wpts, *pnp_K, *pnp_T0; double *pnp_T;
    uint8_t *pnp_outl, *pnp_rem; int32_t *pnp_ok; uint64_t pnp_T_bytes;
    // keyframe detector
    double *det_thresh; const float *det_cur; const int32_t *det_img; int32_t *det_nout; float *det_out;
};

struct FeLoopNative {
    ov2_ctx *ctx = nullptr;
    ov2h_feloop_cfg c{};
    std::vector<void *> left, right;
    std::vector<const float *> kps, pri, st_pri;
    std::vector<const uint8_t *> has, st_has;
    ov2_pyr *prev = nullptr;
    long step_no = 0;
};

void *ov2h_feloop_create(void *ctx, const ov2h_feloop_cfg *cfg)
{
    if (!ctx || !cfg || cfg->L <= 0) return nullptr;
    FeLoopNative *f = new FeLoopNative();
    f->ctx = (ov2_ctx *)ctx; f->c = *cfg;
    const int L = cfg->L;
    f->left.assign(cfg->left, cfg->left + L); f->right.assign(cfg->right, cfg->right + L);
    f->kps.assign(cfg->kps, cfg->kps + L); f->pri.assign(cfg->pri, cfg->pri + L); f->st_pri.assign(cfg->st_pri, cfg->st_pri + L);
    f->has.assign(cfg->has, cfg->has + L); f->st_has.assign(cfg->st_has, cfg->st_has + L);
    return f;
}

// runs `steps` frames; a keyframe every kf_every-th frame submits a job to each of the n_pipes Estimator pipelines.
// returns 0 or the first failing status; *n_kf = keyframes in this call
int ov2h_feloop_run(void *h, int steps, int kf_every, void *const *pipes, int n_pipes, int *n_kf)
{
    FeLoopNative *f = (FeLoopNative *)h;
    const ov2h_feloop_cfg &c = f->c;
    ov2_ctx *ctx = f->ctx;
    int kfs = 0;
    for (int it = 0; it < steps; ++it) {
        const int p = (int)(f->step_no % c.L);
        ov2_pyr *cur = nullptr;
        ov2_status s = ov2_pyramid_build_images(ctx, (const ov2_images *)f->left[p], c.win, c.nlvl, c.use_clahe, c.clahe_clip, c.tiles_x,
                                                c.tiles_y, &cur);
        if (s != OV2_OK) return (int)s;
        if (f->prev) {
            s = ov2_klt_tracking_frame_dev(ctx, f->prev, cur, c.win, c.nlvl, c.max_iter, c.eps, c.err_th, c.fb_th, c.n, f->kps[p], f->pri[p],
                                           f->has[p], c.img_idx, c.out_xy, c.out_st, c.p3p, nullptr);
            ov2_pyr_release(f->prev);
            f->prev = nullptr;
            if (s != OV2_OK) { ov2_pyr_release(cur); return (int)s; }
            if (c.pnp) {
                if ((s = ov2_memcpy_d2d(ctx, c.pnp_T, c.pnp_T0, (size_t)c.pnp_T_bytes)) != OV2_OK ||
                    (s = ov2_pnp_solve_batch_dev(ctx, c.B, c.pnp_off, c.pnp_unpx, c.pnp_wpts, nullptr, c.pnp_K, c.pnp_T, 5, 5.9915f, 1, 1,
                                                 c.pnp_outl, c.pnp_rem, c.pnp_ok, nullptr)) != OV2_OK) { ov2_pyr_release(cur); return (int)s; }
            }
        }
        f->prev = cur;
        const bool is_kf = kf_every > 0 && (f->step_no % kf_every) == 0;
        if (is_kf) {
            ov2_pyr *rp = nullptr;
            if ((s = ov2_pyramid_build_images(ctx, (const ov2_images *)f->right[p], c.win, c.nlvl, c.use_clahe, c.clahe_clip, c.tiles_x,
                                              c.tiles_y, &rp)) != OV2_OK) return (int)s;
            s = ov2_stereo_matching_dev(ctx, cur, rp, c.win, c.nlvl, c.max_iter, c.eps, c.err_th, c.fb_th, c.n, f->kps[p], f->st_pri[p],
                                        f->st_has[p], c.img_idx, nullptr, 1, nullptr, nullptr, c.out_xy, c.out_st, nullptr);
            ov2_pyr_release(rp);
            if (s != OV2_OK) return (int)s;
            if (c.detect && (s = ov2_detect_grid_batch_dev(ctx, cur, c.det_cell, OV2_DETECT_MINEIG, c.det_thresh, c.det_ncur, c.det_cur, c.det_img,
                                                           nullptr, nullptr, 1, c.det_nout, c.det_out, c.det_cap)) != OV2_OK) return (int)s;
            for (int k = 0; k < n_pipes; ++k) ov2h_ba_pipeline_submit_all(pipes[k]);
            ++kfs;
        }
        ++f->step_no;
    }
    if (n_kf) *n_kf = kfs;
    return 0;
}

void ov2h_feloop_destroy(void *h)
{
    FeLoopNative *f = (FeLoopNative *)h;
    if (!f) return;
    if (f->prev) ov2_pyr_release(f->prev);
    delete f;
}

}  // extern "C"

// ---- LoopCloser::newKeyframe: a loop closer that lives across keyframes (its detector and vkfids_) ---------------------------------

extern "C" {

void *ov2h_loop_closer_create(void *p, void *ctx, int lcd_p, float nndr, double min_score, int island_size, int nframes_after_lc,
                              int purge, int min_feat_apps, int nransac_iter, float fransac_err)
{
    HostMap *m = (HostMap *)p;
    loop_params(m, nransac_iter, fransac_err);
    LoopCloser *lc = new LoopCloser((ov2_ctx *)ctx, m->st, m->map);
    LCDetectorParams &P = lc->lcd_params_;
    P.p = (unsigned)lcd_p; P.nndr = nndr; P.min_score = min_score; P.island_size = (unsigned)island_size;
    P.nframes_after_lc = (unsigned)nframes_after_lc; P.purge_descriptors = purge != 0; P.min_feat_apps = (unsigned)min_feat_apps;
    return lc;
}

void ov2h_loop_closer_destroy(void *h) { delete (LoopCloser *)h; }

// out[10]: skipped, image id, detector status, train image id, candidate kfid, candidate used by the 2D-2D half, its branch,
// pairs it passed on, branch of the 2D-3D half, pairs at its end; stats[13] as ov2h_loop_process (zeros without a candidate).
// Returns 0 or a negative ov2_status
int ov2h_loop_new_keyframe(void *h, int kfid, unsigned long long seed, int *out, int *stats)
{
    LoopCloser *lc = (LoopCloser *)h;
    LoopNewKeyframeResult r;
    lc->last_ = LoopStats();
    const ov2_status s = lc->newKeyframe(kfid, (uint64_t)seed, r);
    lc->last_closed_ = r.closed;
    if (s != OV2_OK) return (int)s;
    out[0] = r.skipped ? 1 : 0; out[1] = r.image_id; out[2] = (int)r.det.status; out[3] = (int)r.det.train_id; out[4] = r.cand_kfid;
    out[5] = r.matched.lckfid; out[6] = r.matched.branch; out[7] = (int)r.matched.vkplmids.size(); out[8] = r.verified.branch;
    out[9] = (int)r.verified.vkplmids.size();
    const LoopStats &L = lc->last_;
    const int st[13] = {L.pairs, L.knn_pairs, L.epi_pairs, L.knn_calls, L.epi_calls, L.p3p_pairs, L.refine_pairs, L.track_pairs, L.pnp_pairs,
                        L.p3p_calls, L.refine_calls, L.track_calls, L.pnp_calls};
    std::copy(st, st + 13, stats);
    return 0;
}

void ov2h_loop_set_brief_pattern(void *h, const int8_t *pattern256x4) { ((LoopCloser *)h)->setBriefPattern(pattern256x4); }

// room per image of the first detect call of extraKeypoints (2048 by default)
void ov2h_loop_set_extra_cap(void *h, int cap) { ((LoopCloser *)h)->extra_out_cap_ = cap; }

// the closer's detector (null before its first keyframe) for ov2h_lcd_counts / ov2h_lcd_trace; the closer keeps owning it
// LoopCloser::close_loops_: newKeyframe(s) go on to closeLoop(s) on an LV_ACCEPTED result
void ov2h_loop_closer_set_close(void *h, int on) { ((LoopCloser *)h)->close_loops_ = on != 0; }

// `closed` of the closer's last ov2h_loop_new_keyframe result, as a row of ov2h_loop_close (an untouched LoopCloseResult when
// nothing was closed); stats[3] = last_close_
int ov2h_loop_closer_closed(void *h, int cap, int *ints, double *dbl, int *merged, int *stats)
{
    LoopCloser *lc = (LoopCloser *)h;
    stats[0] = lc->last_close_.jobs; stats[1] = lc->last_close_.graphs; stats[2] = lc->last_close_.solve_calls;
    return pack_close(lc->last_closed_, ints, dbl, cap, merged) ? 0 : (int)OV2_ERR_INVALID;
}

void *ov2h_loop_closer_detector(void *h) { return ((LoopCloser *)h)->plcdetector_.get(); }

// LoopCloser::extraKeypoints for B closers (h[k], kfid[k], image b[k] of pyr).  counts: B x 5 = skipped, nbkps, mask points,
// keypoints after retainBest, keypoints described; mask_xy / add_xy: B x cap x 2, add_resp: B x cap, add_desc: B x cap x 32 (a
// job with more than cap mask points or keypoints: OV2_ERR_INVALID, counts still written); stats[2]: detect and describe calls
int ov2h_loop_extra_keypoints(int B, void *const *h, const int *kfid, void *pyr, const int *b, int cap, int *counts, float *mask_xy,
                              float *add_xy, uint8_t *add_resp, uint8_t *add_desc, int *stats)
{
    if (B <= 0 || !h || !h[0]) return (int)OV2_ERR_INVALID;
    std::vector<LoopExtraJob> jobs((size_t)B);
    for (int k = 0; k < B; ++k) { jobs[k].closer = (LoopCloser *)h[k]; jobs[k].kfid = kfid[k]; jobs[k].b = b[k]; }
    LoopExtraStats es;
    const ov2_status s = LoopCloser::extraKeypoints(jobs[0].closer->ctx_, (const ov2_pyr *)pyr, jobs, es);
    stats[0] = es.detect_calls; stats[1] = es.describe_calls;
    if (s != OV2_OK) return (int)s;
    bool fits = true;
    for (int k = 0; k < B; ++k) {
        const LoopExtraJob &J = jobs[k];
        const int c[5] = {J.skipped ? 1 : 0, J.nbkps, (int)J.mask_px.size(), J.n_detected, (int)J.add_px.size()};
        std::copy(c, c + 5, counts + 5 * k);
        if ((int)J.mask_px.size() > cap || (int)J.add_px.size() > cap) { fits = false; continue; }
        for (size_t i = 0; i < J.mask_px.size(); ++i) { mask_xy[((size_t)k * cap + i) * 2] = J.mask_px[i].x; mask_xy[((size_t)k * cap + i) * 2 + 1] = J.mask_px[i].y; }
        for (size_t i = 0; i < J.add_px.size(); ++i) { add_xy[((size_t)k * cap + i) * 2] = J.add_px[i].x; add_xy[((size_t)k * cap + i) * 2 + 1] = J.add_px[i].y; }
        std::copy(J.add_resp.begin(), J.add_resp.end(), add_resp + (size_t)k * cap);
        std::copy(J.add_descs.begin(), J.add_descs.end(), add_desc + (size_t)k * cap * 32);
    }
    return fits ? 0 : (int)OV2_ERR_INVALID;
}

// LoopCloser::newKeyframes: out B x 13 = the ten of ov2h_loop_new_keyframe, then nbkps, extra keypoints described, descriptor
// rows the detector received; stats B x 13 as there; extra_stats[2]: detect and describe calls of the step
int ov2h_loop_new_keyframes_img(int B, void *const *h, const int *kfid, const unsigned long long *seeds, void *pyr, const int *b, int *out,
                                int *stats, int *extra_stats)
{
    if (B <= 0 || !h) return (int)OV2_ERR_INVALID;
    std::vector<LoopCloser *> lcs((LoopCloser *const *)h, (LoopCloser *const *)h + B);
    std::vector<LoopNewKeyframeResult> res;
    LoopExtraStats es;
    const ov2_status s = LoopCloser::newKeyframes(lcs, std::vector<int>(kfid, kfid + B), std::vector<uint64_t>(seeds, seeds + B),
                                                  (const ov2_pyr *)pyr, std::vector<int>(b, b + B), res, &es);
    extra_stats[0] = es.detect_calls; extra_stats[1] = es.describe_calls;
    if (s != OV2_OK) return (int)s;
    for (int k = 0; k < B; ++k) {
        const LoopNewKeyframeResult &r = res[k];
        const int o[13] = {r.skipped ? 1 : 0, r.image_id, (int)r.det.status, (int)r.det.train_id, r.cand_kfid, r.matched.lckfid, r.matched.branch,
                           (int)r.matched.vkplmids.size(), r.verified.branch, (int)r.verified.vkplmids.size(), r.nbkps, r.n_extra, r.n_descs};
        std::copy(o, o + 13, out + 13 * k);
        const LoopStats &L = lcs[k]->last_;
        const int st[13] = {L.pairs, L.knn_pairs, L.epi_pairs, L.knn_calls, L.epi_calls, L.p3p_pairs, L.refine_pairs, L.track_pairs, L.pnp_pairs,
                            L.p3p_calls, L.refine_calls, L.track_calls, L.pnp_calls};
        std::copy(st, st + 13, stats + 13 * k);
    }
    return 0;
}

// LoopCloser::newKeyframe with the keyframe's raw image: one row of ov2h_loop_new_keyframes_img
int ov2h_loop_new_keyframe_img(void *h, int kfid, unsigned long long seed, void *pyr, int b, int *out, int *stats, int *extra_stats)
{
    return ov2h_loop_new_keyframes_img(1, &h, &kfid, &seed, pyr, &b, out, stats, extra_stats);
}

}  // extern "C"

// ---- loop detector (ov2_lcd.hpp): create with parameters, process / process_batch, and what the last call did -------------

extern "C" {

// ctx may be null: the host brute-force back end
void *ov2h_lcd_create(void *ctx, int p, float nndr, double min_score, int island_size, int nframes_after_lc, int purge, int min_feat_apps)
{
    LCDetectorParams P;
    P.p = (unsigned)p; P.nndr = nndr; P.min_score = min_score; P.island_size = (unsigned)island_size;
    P.nframes_after_lc = (unsigned)nframes_after_lc; P.purge_descriptors = purge != 0; P.min_feat_apps = (unsigned)min_feat_apps;
    return new LCDetector((ov2_ctx *)ctx, P);
}

void ov2h_lcd_destroy(void *h) { delete (LCDetector *)h; }

// status / train_id: B each.  Returns 0 or a negative ov2_status
int ov2h_lcd_process_batch(int B, void *const *h, const unsigned *image_id, const uint8_t *const *descs, const int *n, int *status,
                           int *train_id)
{
    std::vector<LCDetectorResult> r((size_t)std::max(B, 0));
    const ov2_status s = LCDetector::processBatch(B, (LCDetector *const *)h, image_id, descs, n, r.data());
    if (s != OV2_OK) return (int)s;
    for (int b = 0; b < B; ++b) { status[b] = (int)r[b].status; train_id[b] = (int)r[b].train_id; }
    return 0;
}

int ov2h_lcd_process(void *h, unsigned image_id, const uint8_t *descs, int n, int *status, int *train_id)
{
    return ov2h_lcd_process_batch(1, &h, &image_id, &descs, &n, status, train_id);
}

// out[10]: images, live words of the host index, device slots / live words / compactions, and of the last process call the
// number of add matches, query matches, words added, words purged, islands (scores: one per image)
void ov2h_lcd_counts(void *h, int *out)
{
    const LCDetector *d = (const LCDetector *)h;
    const LCDetectorTrace &t = d->trace();
    out[0] = (int)d->index().numImages(); out[1] = (int)d->index().numDescriptors();
    d->index().deviceCounts(&out[2], &out[3], &out[4]);
    out[5] = (int)t.add_matches.size(); out[6] = (int)t.matches.size(); out[7] = (int)t.added.size(); out[8] = (int)t.purged.size();
    out[9] = (int)t.islands.size();
}

// the trace of the last process call into arrays sized from ov2h_lcd_counts: matches as (query row, word id, distance) int
// triples, islands as (img_id, min, max) + score; returns the number of scores written (<= cap_scores)
int ov2h_lcd_trace(void *h, int *add_matches, int *matches, int *added, int *purged, double *scores, int cap_scores, int *islands,
                   double *island_scores)
{
    const LCDetectorTrace &t = ((const LCDetector *)h)->trace();
    for (size_t i = 0; i < t.add_matches.size(); ++i) { add_matches[3 * i] = t.add_matches[i].queryIdx; add_matches[3 * i + 1] = t.add_matches[i].trainIdx; add_matches[3 * i + 2] = (int)t.add_matches[i].distance; }
    for (size_t i = 0; i < t.matches.size(); ++i) { matches[3 * i] = t.matches[i].queryIdx; matches[3 * i + 1] = t.matches[i].trainIdx; matches[3 * i + 2] = (int)t.matches[i].distance; }
    for (size_t i = 0; i < t.added.size(); ++i) added[i] = (int)t.added[i];
    for (size_t i = 0; i < t.purged.size(); ++i) purged[i] = (int)t.purged[i];
    const int ns = (int)std::min(t.scores.size(), (size_t)std::max(cap_scores, 0));
    for (int i = 0; i < ns; ++i) scores[i] = t.scores[i];
    for (size_t i = 0; i < t.islands.size(); ++i) {
        islands[3 * i] = (int)t.islands[i].img_id; islands[3 * i + 1] = (int)t.islands[i].min_img_id; islands[3 * i + 2] = (int)t.islands[i].max_img_id;
        island_scores[i] = t.islands[i].score;
    }
    return ns;
}

}  // extern "C"
