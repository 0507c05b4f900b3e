// match.hip -- keyframe descriptors and map matching (first half):
//   brief_kernel   FeatureExtractor::describeBRIEF src/feature_extractor.cpp:224-285 (cv::xfeatures2d::BriefDescriptorExtractor:
//                  32 bytes, patch 48, 9 x 9 box sums at the rounded keypoint) with a caller-supplied test table
//   match_cand_kernel<false>  Mapper::matchToMap src/mapper.cpp:576-774 for B frames, one local map each
//                  (ov2_match_batch_input; ov2_match_input is its B = 1 case)
//   match_cand_kernel<true>   LoopCloser::matchToMap src/loop_closer.cpp:586-763 for B candidate pairs (ov2_loop_match_input)
// Integer box sums and Hamming distances => bit-exact against the oracle; the float gates are evaluated in its order.
#include <type_traits>

#include "ov2_internal.h"
#include "ov2_cam.h"
#include "ov2_se3.h"

namespace {

enum { K_BRIEF = OV2_K_MAP + 4, K_MATCH = OV2_K_MAP + 5, K_LOOP_MATCH = OV2_K_MAP + 15 };
enum { MATCH_WAVES = 4 };   // candidates per workgroup of match_cand_kernel

// one wave per keypoint: the 57 x 57 pixels the 256 tests can touch are staged in LDS, lane l evaluates tests l, l + 64, ...
__global__ __launch_bounds__(64) void brief_kernel(ov2_pyr_view pv, int n, const float2 *__restrict__ pts,
                                                   const int *__restrict__ img_idx, const signed char *__restrict__ pattern,
                                                   unsigned char *__restrict__ desc, unsigned char *__restrict__ valid, int b0)
{
    __shared__ unsigned char patch[57 * 60];
    __shared__ unsigned bits[8];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const ov2_level_desc &L = pv.lv[0];
    const int w = L.w, h = L.h, b = img_idx ? img_idx[i] : b0;
    const float x = pts[i].x, y = pts[i].y;
    const int border = 28;   // PATCH_SIZE / 2 + KERNEL_SIZE / 2
    const bool ok = (w > 2 * border && h > 2 * border) && x >= (float)border && x < (float)(w - border) && y >= (float)border &&
                    y < (float)(h - border);
    if (!ok) {
        if (lane < 32) desc[(size_t)i * 32 + lane] = 0;
        if (lane == 0) valid[i] = 0;
        return;
    }
    const int px = (int)((double)x + 0.5), py = (int)((double)y + 0.5);
    const unsigned char *img = pv.base + L.img_off + L.img_bstride * b + (size_t)pv.pad * L.istride + OV2_LM;
    for (int k = lane; k < 57 * 57; k += 64) {
        const int r = k / 57, c = k - r * 57;
        patch[r * 60 + c] = img[(size_t)(py - 28 + r) * L.istride + (px - 28 + c)];
    }
    if (lane < 8) bits[lane] = 0;
    __syncthreads();
    for (int k = lane; k < 256; k += 64) {
        const signed char *t = pattern + 4 * k;
        int a = 0, bsum = 0;
        const int ya = 28 + t[0], xa = 28 + t[1], yb = 28 + t[2], xb = 28 + t[3];
        for (int dy = -4; dy <= 4; ++dy)
            for (int dx = -4; dx <= 4; ++dx) {
                a += patch[(ya + dy) * 60 + xa + dx];
                bsum += patch[(yb + dy) * 60 + xb + dx];
            }
        if (a < bsum) atomicOr(&bits[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    if (lane < 32) {   // byte j holds tests 8 j .. 8 j + 7, the first one in its most significant bit
        const unsigned wv = bits[lane >> 2] >> ((lane & 3) * 8);
        unsigned char o = 0;
        for (int q = 0; q < 8; ++q) o |= (unsigned char)(((wv >> q) & 1u) << (7 - q));
        desc[(size_t)i * 32 + lane] = o;
    }
    if (lane == 0) valid[i] = 1;
}

// The arrays of a matcher call: the device twin of ov2_match_batch_input and of ov2_loop_match_input (cam normalised, with
// the call's K), and on the host the form both are checked and staged in (host pointers then).  Mapper's extras stay null
// for the loop closer, the loop closer's for Mapper.
struct match_dev {
    ov2_cam_model cam;
    int B, n_kp, n_cand, img_w, img_h, cell, nbw, ncells;
    const double *Twc; const int *kp_off, *cand_off;
    const float2 *kp_px; const int *kp_desc_ptr; const unsigned char *kp_descs; const int *kp_kf_ptr, *kp_kfids;
    const int *grid_ptr, *grid_kp;
    const double *cand_wpt; const int *cand_desc_ptr; const unsigned char *cand_descs; const int *cand_kf_ptr, *cand_kfids;
    const int *nb3dkps, *kf_off; const float2 *kp_kf_px; const double *kf_Twc;   // Mapper
    const unsigned char *kp_matched;                                               // loop closer
};

__device__ inline void world_to_cam(const double *Twc, const double *p, double c[3])
{
    double R[9];
    ov2se3::pose_R(Twc, R);
    const double d[3] = {p[0] - Twc[0], p[1] - Twc[1], p[2] - Twc[2]};
    for (int r = 0; r < 3; ++r) c[r] = R[r] * d[0] + R[3 + r] * d[1] + R[6 + r] * d[2];
}

__device__ inline int hamming32(const unsigned char *a, const unsigned char *b)
{
    const unsigned long long *pa = reinterpret_cast<const unsigned long long *>(a), *pb = reinterpret_cast<const unsigned long long *>(b);
    return __popcll(pa[0] ^ pb[0]) + __popcll(pa[1] ^ pb[1]) + __popcll(pa[2] ^ pb[2]) + __popcll(pa[3] ^ pb[3]);
}

// true when two ascending keyframe lists share an entry (the map point and the keypoint's map point are co-observed)
__device__ inline bool kf_lists_meet(const int *a, int a0, int a1, const int *b, int b0, int b1)
{
    while (a0 < a1 && b0 < b1) {
        const int ka = a[a0], kb = b[b0];
        if (ka == kb) return true;
        if (ka < kb) ++a0; else ++b0;
    }
    return false;
}

// MapPoint::computeMinDescDist: the minimum Hamming distance over both descriptor sets
__device__ inline float min_desc_dist(const unsigned char *da, int a0, int a1, const unsigned char *db, int b0, int b1)
{
    float dmin = 1000.f;
    for (int i = a0; i < a1; ++i)
        for (int j = b0; j < b1; ++j) {
            const float hd = (float)hamming32(da + 32 * (size_t)i, db + 32 * (size_t)j);
            if (hd < dmin) dmin = hd;
        }
    return dmin;
}

// What Mapper::matchToMap and LoopCloser::matchToMap share once a map point is projected to (px, py): the keypoints of the
// 2 x 2 cells of Frame::getSurroundingKeypoints(cv::Point2f) (src/frame.cpp:624-650), 64 at a time, one per lane --
// dist_of(grid entry) gives the lane's descriptor distance or < 0 where the keypoint is not a candidate --, the best / second
// best bookkeeping replayed in the reference's order (wave-uniform; it breaks ties by position) and the 0.9 ratio.
// Returns the grid entry of the match or -1, its distance in bestdist.  The whole wave must call it.
template <class DistOf>
__device__ inline int match_walk_cells(float px, float py, int cell, int nbw, int ncells, const int *__restrict__ grid_ptr,
                                       const int *__restrict__ grid_kp, int lane, float mindist, float &bestdist, DistOf dist_of)
{
    int bestid = -1, secid = -1;
    float secdist = mindist;
    bestdist = mindist;
    const int rkp = (int)floorf(py / (float)cell), ckp = (int)floorf(px / (float)cell);
    for (int cellk = 0; cellk < 4; ++cellk) {
        const int r = rkp - 1 + (cellk >> 1), cc = ckp - 1 + (cellk & 1);
        const int idx = r * nbw + cc;
        if (r < 0 || cc < 0 || idx >= ncells) continue;
        const int g0 = grid_ptr[idx], g1 = grid_ptr[idx + 1];
        for (int base = g0; base < g1; base += 64) {
            const int g = base + lane;
            float dist = -1.f;   // < 0: this keypoint is not a candidate
            int k = -1;
            if (g < g1) {
                k = grid_kp[g];
                dist = dist_of(k);
            }
            const int cnt = min(64, g1 - base);
            for (int q = 0; q < cnt; ++q) {
                const float dq = __shfl(dist, q);
                const int kq = __shfl(k, q);
                if (dq < 0.f) continue;
                if (dq <= bestdist) { secdist = bestdist; secid = bestid; bestdist = dq; bestid = kq; }
                else if (dq <= secdist) { secdist = dq; secid = kq; }
            }
        }
    }
    if (bestid != -1 && secid != -1 && 0.9 * (double)secdist < (double)bestdist) bestid = -1;
    return bestid;
}

// The per-keypoint test of Mapper::matchToMap (src/mapper.cpp:676-721) for candidate c (descriptors cd0 .. cd1, world point wpt,
// projected to (px, py)) and keypoint k, both indices into the flat arrays of M (match_dev): pixel gate,
// descriptors present, co-observation test, mean reprojection distance in the keypoint's keyframes -- kf_Twc / n_kf are the
// pose table those ids index, ids outside it are skipped, 0 / 0 compares false --, then the minimum Hamming distance over the
// two descriptor sets.  < 0: the keypoint is not a candidate.
template <class Arrays>
__device__ inline float match_kp_dist(const Arrays &M, int c, int k, int cd0, int cd1, const double *wpt, float px, float py,
                                      float dmaxpxdist, const double *kf_Twc, int n_kf)
{
    const float dx = px - M.kp_px[k].x, dy = py - M.kp_px[k].y;
    const float pxdist = (float)sqrt((double)dx * dx + (double)dy * dy);
    const int kd0 = M.kp_desc_ptr[k], kd1 = M.kp_desc_ptr[k + 1];
    if (pxdist > dmaxpxdist || kd1 <= kd0) return -1.f;
    if (kf_lists_meet(M.cand_kfids, M.cand_kf_ptr[c], M.cand_kf_ptr[c + 1], M.kp_kfids, M.kp_kf_ptr[k], M.kp_kf_ptr[k + 1])) return -1.f;
    float coprojpx = 0.f;   // mean reprojection distance in the keypoint's keyframes (src/mapper.cpp:700-719)
    int nbcokp = 0;
    for (int e = M.kp_kf_ptr[k]; e < M.kp_kf_ptr[k + 1]; ++e) {
        const int kfid = M.kp_kfids[e];
        if (kfid < 0 || kfid >= n_kf) continue;
        double cp[3];
        world_to_cam(kf_Twc + 7 * (size_t)kfid, wpt, cp);
        float qx, qy;
        ov2_cam_project_dist(M.cam, cp, qx, qy);
        const float ex = M.kp_kf_px[e].x - qx, ey = M.kp_kf_px[e].y - qy;
        coprojpx = (float)((double)coprojpx + sqrt((double)ex * ex + (double)ey * ey));
        ++nbcokp;
    }
    if (coprojpx / (float)nbcokp > dmaxpxdist) return -1.f;
    return min_desc_dist(M.cand_descs, cd0, cd1, M.kp_descs, kd0, kd1);
}

// The per-keypoint test of LoopCloser::matchToMap (src/loop_closer.cpp:672-709), arguments as match_kp_dist: the matched mask
// first, pixel gate, descriptors present, co-observation test, minimum Hamming distance; no mean-reprojection gate.
__device__ inline float loop_kp_dist(const match_dev &M, int c, int k, int cd0, int cd1, float px, float py, float dmaxpxdist)
{
    if (M.kp_matched[k]) return -1.f;                                               // :672-675
    const float dx = px - M.kp_px[k].x, dy = py - M.kp_px[k].y;
    const float pxdist = (float)sqrt((double)dx * dx + (double)dy * dy);
    const int kd0 = M.kp_desc_ptr[k], kd1 = M.kp_desc_ptr[k + 1];
    if (pxdist > dmaxpxdist || kd1 <= kd0) return -1.f;                             // :683, :690-695
    if (kf_lists_meet(M.cand_kfids, M.cand_kf_ptr[c], M.cand_kf_ptr[c + 1], M.kp_kfids, M.kp_kf_ptr[k], M.kp_kf_ptr[k + 1])) return -1.f;
    return min_desc_dist(M.cand_descs, cd0, cd1, M.kp_descs, kd0, kd1);             // :709
}

// One wave per candidate map point, MATCH_WAVES candidates per workgroup (the waves share nothing, so the result does not
// depend on it).  The frame -- for the loop closer: the pair -- of a candidate is found in the B + 1 offsets; its pose, its
// grid and its keypoint block follow from it.  Then the gates, the neighbouring keypoints 64 at a time, one per lane, and the
// best / second-best bookkeeping replayed in the reference's order (match_walk_cells).  The winner goes to the keypoint's slot
// by a 64-bit atomicMin on (distance, ~candidate index within its frame): smallest distance, later candidate on ties.
// LOOP = false, Mapper::matchToMap: match_kp_dist on the frame's keyframe-pose block, the pixel gate doubled under 30 3-D
// keypoints (src/mapper.cpp:599-602).  LOOP = true, LoopCloser::matchToMap: loop_kp_dist.
template <bool LOOP>
__global__ __launch_bounds__(64 * MATCH_WAVES) void match_cand_kernel(match_dev M, float fmaxprojerr, float mindist, float view_th,
                                                                     unsigned long long *__restrict__ kp_best)
{
    const int c = blockIdx.x * MATCH_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= M.n_cand) return;
    int lo = 0, hi = M.B;   // the frame b with cand_off[b] <= c < cand_off[b + 1] (empty frames are stepped over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (M.cand_off[mid] <= c) lo = mid; else hi = mid;
    }
    const int b = lo, c0 = M.cand_off[b], k0 = M.kp_off[b], nkp = M.kp_off[b + 1] - k0;
    if (nkp <= 0) return;
    const int cd0 = M.cand_desc_ptr[c], cd1 = M.cand_desc_ptr[c + 1];
    if (cd1 == cd0) return;
    const double *wpt = M.cand_wpt + 3 * (size_t)c;
    double campt[3];
    world_to_cam(M.Twc + 7 * (size_t)b, wpt, campt);
    if (campt[2] < 0.1) return;
    const float view_angle = (float)(campt[2] / sqrt(campt[0] * campt[0] + campt[1] * campt[1] + campt[2] * campt[2]));
    if (fabsf(view_angle) < view_th) return;
    float px, py;
    ov2_cam_project_dist(M.cam, campt, px, py);
    if (!(px >= 0 && py >= 0 && px < (float)M.img_w && py < (float)M.img_h)) return;
    float dmaxpxdist = fmaxprojerr;
    const double *kf_Twc = nullptr;
    int n_kf = 0;
    if constexpr (!LOOP) {
        if (M.nb3dkps[b] < 30) dmaxpxdist = fmaxprojerr * 2.f;
        const int kf0 = M.kf_off[b];
        n_kf = M.kf_off[b + 1] - kf0;
        kf_Twc = M.kf_Twc + 7 * (size_t)kf0;
    }
    float bestdist;
    const int bestid = match_walk_cells(px, py, M.cell, M.nbw, M.ncells, M.grid_ptr + (size_t)b * M.ncells, M.grid_kp, lane, mindist, bestdist,
                                        [&](int kl) {
        if ((unsigned)kl >= (unsigned)nkp) return -1.f;   // (the host form refuses such a grid; the _dev form cannot look)
        if constexpr (LOOP) return loop_kp_dist(M, c, k0 + kl, cd0, cd1, px, py, dmaxpxdist);
        else return match_kp_dist(M, c, k0 + kl, cd0, cd1, wpt, px, py, dmaxpxdist, kf_Twc, n_kf);
    });
    if (bestid < 0) return;
    if (lane == 0)   // Hamming distances are small integers: exact in the key
        atomicMin(&kp_best[k0 + bestid],
                  ((unsigned long long)(unsigned)(int)bestdist << 32) | (unsigned long long)(0xffffffffu - (unsigned)(c - c0)));
}

__global__ void match_out_kernel(int n_kp, const unsigned long long *__restrict__ kp_best, int *__restrict__ match_cand,
                                 float *__restrict__ match_dist)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kp) return;
    const unsigned long long v = kp_best[k];
    if (v == ~0ull) { match_cand[k] = -1; match_dist[k] = 0.f; }
    else { match_cand[k] = (int)(0xffffffffu - (unsigned)(v & 0xffffffffull)); match_dist[k] = (float)(unsigned)(v >> 32); }
}

}  // namespace

extern "C" ov2_status ov2_describe_brief_dev(ov2_ctx *c, const ov2_pyr *pyr, int n, const float *d_pts_xy, const int32_t *d_img_idx,
                                             const int8_t *d_pattern, uint8_t *d_desc, uint8_t *d_valid)
{
    if (!c) return OV2_ERR_INVALID;
    if (n == 0) return OV2_OK;
    if (n < 0 || !pyr || !d_pts_xy || !d_pattern || !d_desc || !d_valid) return ov2_set_err(c, OV2_ERR_INVALID, "null/negative argument");
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_status s = ov2_pyr_wait_ready(c, pyr);
    if (s != OV2_OK) return s;
    OV2_LAUNCH(c, K_BRIEF, brief_kernel, dim3(n), dim3(64), 0, c->stream, pyr->buf->view, n, reinterpret_cast<const float2 *>(d_pts_xy),
               d_img_idx, reinterpret_cast<const signed char *>(d_pattern), d_desc, d_valid, 0);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

// host-pointer form; img_idx == nullptr: every point lies in image b
static ov2_status describe_brief_host(ov2_ctx *c, const ov2_pyr *pyr, int b, int n, const float *pts_xy, const int32_t *img_idx,
                                      const int8_t *pattern, uint8_t *desc, uint8_t *valid)
{
    if (!c) return OV2_ERR_INVALID;
    if (n == 0) return OV2_OK;
    if (n < 0 || !pyr || !pts_xy || !pattern || !desc || !valid) return ov2_set_err(c, OV2_ERR_INVALID, "null/negative argument");
    if (b < 0 || b >= pyr->buf->batch) return ov2_set_err(c, OV2_ERR_INVALID, "image %d outside the pyramid batch", b);
    if (img_idx)
        for (int k = 0; k < n; ++k)
            if (img_idx[k] < 0 || img_idx[k] >= pyr->buf->batch)
                return ov2_set_err(c, OV2_ERR_INVALID, "image %d outside the pyramid batch", (int)img_idx[k]);
    for (int k = 0; k < 1024; ++k)
        if (pattern[k] < -24 || pattern[k] > 24) return ov2_set_err(c, OV2_ERR_INVALID, "BRIEF test offset %d outside [-24, 24]", (int)pattern[k]);
    void *hs = nullptr, *ds = nullptr;
    const size_t npts = (size_t)n * 8, nb = npts + (img_idx ? (size_t)n * 4 : 0), need = nb + 1024 + (size_t)n * 33 + 64;
    ov2_status s = ov2_staging(c, need, &hs, &ds);
    if (s != OV2_OK) return s;
    char *h = (char *)hs, *d = (char *)ds;
    memcpy(h, pts_xy, npts);
    if (img_idx) memcpy(h + npts, img_idx, (size_t)n * 4);
    memcpy(h + nb, pattern, 1024);
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipMemcpyAsync(d, h, nb + 1024, hipMemcpyHostToDevice, c->stream));
    if ((s = ov2_pyr_wait_ready(c, pyr)) != OV2_OK) return s;
    uint8_t *d_desc = (uint8_t *)(d + nb + 1024), *d_valid = d_desc + (size_t)n * 32;
    OV2_LAUNCH(c, K_BRIEF, brief_kernel, dim3(n), dim3(64), 0, c->stream, pyr->buf->view, n, reinterpret_cast<const float2 *>(d),
               img_idx ? reinterpret_cast<const int32_t *>(d + npts) : nullptr, reinterpret_cast<const signed char *>(d + nb), d_desc, d_valid, b);
    OV2_HIP(c, hipMemcpyAsync(h + nb + 1024, d_desc, (size_t)n * 33, hipMemcpyDeviceToHost, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(desc, h + nb + 1024, (size_t)n * 32);
    memcpy(valid, h + nb + 1024 + (size_t)n * 32, (size_t)n);
    return OV2_OK;
}

extern "C" ov2_status ov2_describe_brief(ov2_ctx *c, const ov2_pyr *pyr, int b, int n, const float *pts_xy, const int8_t *pattern,
                                         uint8_t *desc, uint8_t *valid)
{
    return describe_brief_host(c, pyr, b, n, pts_xy, nullptr, pattern, desc, valid);
}

extern "C" ov2_status ov2_describe_brief_batch(ov2_ctx *c, const ov2_pyr *pyr, int n, const float *pts_xy, const int32_t *img_idx,
                                               const int8_t *pattern, uint8_t *desc, uint8_t *valid)
{
    if (c && n > 0 && !img_idx) return ov2_set_err(c, OV2_ERR_INVALID, "null image indices");
    return describe_brief_host(c, pyr, 0, n, pts_xy, img_idx, pattern, desc, valid);
}

// ---- Mapper::matchToMap (src/mapper.cpp:576-774) for B frames, one local map each, and LoopCloser::matchToMap
// ---- (src/loop_closer.cpp:586-763) for B candidate pairs: one path, `loop` picks the rules ------------------------------

namespace {

// thresholds exactly as the reference forms them (src/mapper.cpp:586-598, :651): the quotients are Mapper's
void match_thresholds(const double *K, int img_w, int img_h, float fdistratio, float &mindist, float &view_th)
{
    const float vfov = (float)(0.5 * img_h / K[1]), hfov = (float)(0.5 * img_w / K[0]);
    const float maxradfov = hfov > vfov ? atanf(hfov) : atanf(vfov);
    view_th = cosf(maxradfov);
    mindist = (float)((double)(32.f * fdistratio) * 8.);
}

// thresholds exactly as the reference forms them (src/loop_closer.cpp:595-607, :656): the products and the one-sided atan
// are the reference's
void loop_match_thresholds(const double *K, int img_w, int img_h, float fdistratio, float &mindist, float &view_th)
{
    const float vfov = (float)(0.5 * (double)img_h * K[1]), hfov = (float)(0.5 * (double)img_w * K[0]);
    float maxradfov = 0.f;
    if (hfov > vfov) maxradfov = atanf(hfov);
    else maxradfov = atanf(hfov);
    view_th = cosf(maxradfov);
    mindist = (float)((double)(32.f * fdistratio) * 8.);
}

// the arrays of a call from either public input; a null input reads as a negative count, which every path refuses first
template <class In>
match_dev match_arrays(const In *in)
{
    match_dev M{};
    M.B = -1;
    if (!in) return M;
    M.cam = ov2_cam_normalised(in->cam);
    for (int i = 0; i < 4; ++i) M.cam.K[i] = in->K[i];   // one set of intrinsics: the call's
    M.B = in->B; M.n_kp = in->n_kp; M.n_cand = in->n_cand; M.img_w = in->img_w; M.img_h = in->img_h; M.cell = in->cell;
    M.Twc = in->Twc; M.kp_off = in->kp_off; M.cand_off = in->cand_off;
    M.kp_px = (const float2 *)in->kp_px; M.kp_desc_ptr = in->kp_desc_ptr; M.kp_descs = in->kp_descs;
    M.kp_kf_ptr = in->kp_kf_ptr; M.kp_kfids = in->kp_kfids; M.grid_ptr = in->grid_ptr; M.grid_kp = in->grid_kp;
    M.cand_wpt = in->cand_wpt; M.cand_desc_ptr = in->cand_desc_ptr; M.cand_descs = in->cand_descs; M.cand_kf_ptr = in->cand_kf_ptr;
    M.cand_kfids = in->cand_kfids;
    if constexpr (std::is_same_v<In, ov2_loop_match_input>) M.kp_matched = in->kp_matched;
    else { M.nb3dkps = in->nb3dkps; M.kf_off = in->kf_off; M.kp_kf_px = (const float2 *)in->kp_kf_px; M.kf_Twc = in->kf_Twc; }
    return M;
}

// The _dev entry points: every array of M is a device pointer.  Checks, the 0xff fill of the work array, the two launches;
// nothing is synchronised.  name: the public entry point, for the messages.
ov2_status match_enqueue(ov2_ctx *c, const char *name, bool loop, match_dev M, float fmaxprojerr, float fdistratio, uint64_t *d_work,
                         int32_t *d_match_cand, float *d_match_dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (M.B < 0 || M.n_kp < 0 || M.n_cand < 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: negative count", name);
    if (M.B == 0 || M.n_kp == 0) return OV2_OK;
    if (M.cell <= 0 || M.img_w <= 0 || M.img_h <= 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: bad image / cell size", name);
    if (!d_work || !d_match_cand || !d_match_dist || !M.kp_off || !M.cand_off || (!loop && !M.kf_off))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", name);
    if (M.n_cand && (!M.Twc || !M.kp_px || !M.kp_desc_ptr || !M.kp_kf_ptr || !M.grid_ptr || !M.cand_wpt || !M.cand_desc_ptr ||
                     !M.cand_kf_ptr || (loop ? !M.kp_matched : !M.nb3dkps)))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: null array", name);
    if (((uintptr_t)M.kp_descs | (uintptr_t)M.cand_descs) & 7)   // descriptors are read 8 bytes at a time
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: descriptor arrays must be 8-byte aligned", name);
    if (M.cam.model < 0 || M.cam.model > 2) return ov2_set_err(c, OV2_ERR_INVALID, "unknown lens model %d", M.cam.model);
    M.nbw = (int)ceilf((float)M.img_w / (float)M.cell);
    M.ncells = M.nbw * (int)ceilf((float)M.img_h / (float)M.cell);
    float mindist, view_th;
    (loop ? loop_match_thresholds : match_thresholds)(M.cam.K, M.img_w, M.img_h, fdistratio, mindist, view_th);
    const int tag = loop ? K_LOOP_MATCH : K_MATCH;
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipMemsetAsync(d_work, 0xff, (size_t)M.n_kp * 8, c->stream));
    if (M.n_cand > 0)
        OV2_LAUNCH(c, tag, loop ? match_cand_kernel<true> : match_cand_kernel<false>, dim3((M.n_cand + MATCH_WAVES - 1) / MATCH_WAVES),
                   dim3(64 * MATCH_WAVES), 0, c->stream, M, fmaxprojerr, mindist, view_th, (unsigned long long *)d_work);
    OV2_LAUNCH(c, tag, match_out_kernel, dim3((M.n_kp + 255) / 256), dim3(256), 0, c->stream, M.n_kp, (const unsigned long long *)d_work,
               d_match_cand, d_match_dist);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

// The host-pointer entry points: every array of M is a host pointer.  Checks of everything the kernel indexes with, one staging
// block [inputs || work | match_cand | match_dist], one upload, match_enqueue, one download and one synchronisation.
ov2_status match_host(ov2_ctx *c, const char *name, bool loop, const match_dev &M, float fmaxprojerr, float fdistratio,
                      int32_t *match_cand, float *match_dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (M.B < 0 || M.n_kp < 0 || M.n_cand < 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: negative count", name);
    const int B = M.B, nkp = M.n_kp, nc = M.n_cand;
    const char *unit = loop ? "pair" : "frame";
    if (B == 0) return OV2_OK;
    if (!M.kp_off || !M.cand_off || (!loop && !M.kf_off)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null offsets", name);
    if (M.kp_off[0] != 0 || M.cand_off[0] != 0 || (!loop && M.kf_off[0] != 0) || M.kp_off[B] != nkp || M.cand_off[B] != nc)
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: offsets do not start at 0 or do not span n_kp / n_cand", name);
    for (int b = 0; b < B; ++b)
        if (M.kp_off[b + 1] < M.kp_off[b] || M.cand_off[b + 1] < M.cand_off[b] || (!loop && M.kf_off[b + 1] < M.kf_off[b]))
            return ov2_set_err(c, OV2_ERR_INVALID, "%s: %s %d has a negative count", name, unit, b);
    if (nkp && (!match_cand || !match_dist)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null output", name);
    for (int k = 0; k < nkp; ++k) { match_cand[k] = -1; match_dist[k] = 0.f; }
    if (nkp == 0 || nc == 0) return OV2_OK;                                  // src/mapper.cpp:580-583, src/loop_closer.cpp:591-593
    if (M.cell <= 0 || M.img_w <= 0 || M.img_h <= 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: bad image / cell size", name);
    if (!M.Twc || !M.kp_px || !M.kp_desc_ptr || !M.kp_kf_ptr || !M.grid_ptr || !M.cand_wpt || !M.cand_desc_ptr || !M.cand_kf_ptr ||
        (loop ? !M.kp_matched : !M.nb3dkps))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: null array", name);
    if (!loop && (M.cam.model < 0 || M.cam.model > 2))   // (the loop closer's form leaves this refusal to match_enqueue)
        return ov2_set_err(c, OV2_ERR_INVALID, "unknown lens model %d", M.cam.model);
    const int nbw = (int)ceilf((float)M.img_w / (float)M.cell), nbh = (int)ceilf((float)M.img_h / (float)M.cell);
    const size_t ncells = (size_t)nbw * nbh, ng_ptr = (size_t)B * ncells + 1;
    // the kernel indexes with these: every prefix array starts at 0 and never decreases, every grid entry lies in its frame
    auto csr_ok = [](const int *p, size_t n) {
        if (p[0] != 0) return false;
        for (size_t i = 0; i < n; ++i) if (p[i + 1] < p[i]) return false;
        return true;
    };
    if (!csr_ok(M.kp_desc_ptr, nkp) || !csr_ok(M.kp_kf_ptr, nkp) || !csr_ok(M.cand_desc_ptr, nc) || !csr_ok(M.cand_kf_ptr, nc) ||
        !csr_ok(M.grid_ptr, ng_ptr - 1))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: a prefix array decreases or does not start at 0", name);
    const size_t n_kpd = (size_t)M.kp_desc_ptr[nkp], n_kpk = (size_t)M.kp_kf_ptr[nkp], n_g = (size_t)M.grid_ptr[ng_ptr - 1];
    const size_t n_cd = (size_t)M.cand_desc_ptr[nc], n_ck = (size_t)M.cand_kf_ptr[nc], n_kf = loop ? 0 : (size_t)M.kf_off[B];
    if ((n_kpd && !M.kp_descs) || (n_kpk && (!M.kp_kfids || (!loop && !M.kp_kf_px))) || (n_g && !M.grid_kp) || (n_cd && !M.cand_descs) ||
        (n_ck && !M.cand_kfids) || (n_kf && !M.kf_Twc))
        return ov2_set_err(c, OV2_ERR_INVALID, "%s: null array", name);
    for (int b = 0; b < B; ++b) {
        const int nb = M.kp_off[b + 1] - M.kp_off[b];
        for (int g = M.grid_ptr[(size_t)b * ncells]; g < M.grid_ptr[(size_t)(b + 1) * ncells]; ++g)
            if (M.grid_kp[g] < 0 || M.grid_kp[g] >= nb)
                return ov2_set_err(c, OV2_ERR_INVALID, "%s: grid entry %d of %s %d outside its %d keypoints", name, M.grid_kp[g], unit, b, nb);
    }
    match_dev D = M;
    auto arrays = [&](auto &&f) {   // every array the call reads, with its size in bytes
        f(D.Twc, (size_t)B * 56); f(D.kp_off, ((size_t)B + 1) * 4); f(D.cand_off, ((size_t)B + 1) * 4);
        f(D.kp_px, (size_t)nkp * 8); f(D.kp_desc_ptr, ((size_t)nkp + 1) * 4); f(D.kp_descs, n_kpd * 32);
        f(D.kp_kf_ptr, ((size_t)nkp + 1) * 4); f(D.kp_kfids, n_kpk * 4); f(D.grid_ptr, ng_ptr * 4); f(D.grid_kp, n_g * 4);
        f(D.cand_wpt, (size_t)nc * 24); f(D.cand_desc_ptr, ((size_t)nc + 1) * 4); f(D.cand_descs, n_cd * 32);
        f(D.cand_kf_ptr, ((size_t)nc + 1) * 4); f(D.cand_kfids, n_ck * 4);
        if (loop) f(D.kp_matched, (size_t)nkp);
        else { f(D.nb3dkps, (size_t)B * 4); f(D.kf_off, ((size_t)B + 1) * 4); f(D.kp_kf_px, n_kpk * 8); f(D.kf_Twc, n_kf * 56); }
    };
    // one staging block, every array 16-byte aligned
    auto pad = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
    size_t o_in = 0;
    arrays([&](auto *&, size_t bytes) { o_in += pad(bytes); });
    const size_t o_best = o_in, o_mc = o_best + pad((size_t)nkp * 8), o_md = o_mc + pad((size_t)nkp * 4), total = o_md + pad((size_t)nkp * 4);
    void *hs = nullptr, *ds = nullptr;
    ov2_status s = ov2_staging(c, total + 64, &hs, &ds);
    if (s != OV2_OK) return s;
    char *h = (char *)hs, *d = (char *)ds;
    size_t off = 0;
    arrays([&](auto *&p, size_t bytes) {   // the array into the block, p to its device copy
        if (bytes) memcpy(h + off, p, bytes);
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(d + off);
        off += pad(bytes);
    });
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipMemcpyAsync(d, h, o_in, hipMemcpyHostToDevice, c->stream));
    s = match_enqueue(c, name, loop, D, fmaxprojerr, fdistratio, (uint64_t *)(d + o_best), (int32_t *)(d + o_mc), (float *)(d + o_md));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(h + o_mc, d + o_mc, (o_md - o_mc) + (size_t)nkp * 4, hipMemcpyDeviceToHost, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(match_cand, h + o_mc, (size_t)nkp * 4);
    memcpy(match_dist, h + o_md, (size_t)nkp * 4);
    return OV2_OK;
}

}  // namespace

// the B = 1 case of ov2_match_to_map_batch
extern "C" ov2_status ov2_match_to_map(ov2_ctx *c, const ov2_match_input *in, float fmaxprojerr, float fdistratio,
                                       int32_t *match_cand, float *match_dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (!in || !match_cand || !match_dist || in->n_kp < 0 || in->n_cand < 0 || in->cell <= 0 || in->img_w <= 0 || in->img_h <= 0)
        return ov2_set_err(c, OV2_ERR_INVALID, "bad ov2_match_input");
    const int32_t kp_off[2] = {0, in->n_kp}, cand_off[2] = {0, in->n_cand}, kf_off[2] = {0, std::max(in->n_kf, 0)};
    ov2_match_batch_input b;
    b.B = 1; b.n_kp = in->n_kp; b.n_cand = in->n_cand; b.img_w = in->img_w; b.img_h = in->img_h; b.cell = in->cell; b.cam = in->cam;
    for (int i = 0; i < 4; ++i) b.K[i] = in->K[i];
    b.Twc = in->Twc; b.nb3dkps = &in->nb3dkps; b.kp_off = kp_off; b.cand_off = cand_off; b.kf_off = kf_off;
    b.kp_px = in->kp_px; b.kp_desc_ptr = in->kp_desc_ptr; b.kp_descs = in->kp_descs; b.kp_kf_ptr = in->kp_kf_ptr; b.kp_kfids = in->kp_kfids;
    b.kp_kf_px = in->kp_kf_px; b.grid_ptr = in->grid_ptr; b.grid_kp = in->grid_kp; b.cand_wpt = in->cand_wpt;
    b.cand_desc_ptr = in->cand_desc_ptr; b.cand_descs = in->cand_descs; b.cand_kf_ptr = in->cand_kf_ptr; b.cand_kfids = in->cand_kfids;
    b.kf_Twc = in->kf_Twc;
    return match_host(c, "ov2_match_to_map", false, match_arrays(&b), fmaxprojerr, fdistratio, match_cand, match_dist);
}

extern "C" ov2_status ov2_match_to_map_batch_dev(ov2_ctx *c, const ov2_match_batch_input *in, float fmaxprojerr, float fdistratio,
                                                 uint64_t *d_work, int32_t *d_match_cand, float *d_match_dist)
{
    return match_enqueue(c, "ov2_match_to_map_batch_dev", false, match_arrays(in), fmaxprojerr, fdistratio, d_work, d_match_cand, d_match_dist);
}

extern "C" ov2_status ov2_match_to_map_batch(ov2_ctx *c, const ov2_match_batch_input *in, float fmaxprojerr, float fdistratio,
                                             int32_t *match_cand, float *match_dist)
{
    return match_host(c, "ov2_match_to_map_batch", false, match_arrays(in), fmaxprojerr, fdistratio, match_cand, match_dist);
}

extern "C" ov2_status ov2_loop_match_to_map_batch_dev(ov2_ctx *c, const ov2_loop_match_input *in, float fmaxprojerr, float fdistratio,
                                                      uint64_t *d_work, int32_t *d_match_cand, float *d_match_dist)
{
    return match_enqueue(c, "ov2_loop_match_to_map_batch_dev", true, match_arrays(in), fmaxprojerr, fdistratio, d_work, d_match_cand, d_match_dist);
}

extern "C" ov2_status ov2_loop_match_to_map_batch(ov2_ctx *c, const ov2_loop_match_input *in, float fmaxprojerr, float fdistratio,
                                                  int32_t *match_cand, float *match_dist)
{
    return match_host(c, "ov2_loop_match_to_map_batch", true, match_arrays(in), fmaxprojerr, fdistratio, match_cand, match_dist);
}

// ---- the matcher's output as ordered pair lists (Mapper::mergeMatches, src/mapper.cpp:556-574) --------------------------

namespace {

#define PAIRS_THREADS 256
// One workgroup per frame.  map_previd_newid is a std::map: the pairs leave it in ascending prevlmid, so a pair's slot is its
// rank among the frame's matched keypoints (ties, which a frame's distinct lmids never give, fall back to the keypoint index:
// the ranks stay a permutation and every write stays inside the frame's segment).  The keys go through LDS 256 at a time.
__global__ __launch_bounds__(PAIRS_THREADS) void match_pairs_kernel(const int *__restrict__ kp_off, const int *__restrict__ cand_off,
                                                                    const int *__restrict__ kp_lmid, const int *__restrict__ cand_lmid,
                                                                    const int *__restrict__ match_cand, int *__restrict__ prev_lmid,
                                                                    int *__restrict__ new_lmid, int *__restrict__ n_pairs)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k0 = kp_off[b], n = kp_off[b + 1] - k0, c0 = cand_off[b], nc = cand_off[b + 1] - c0;
    __shared__ int s_key[PAIRS_THREADS], s_on[PAIRS_THREADS], s_count;
    if (tid == 0) s_count = 0;
    __syncthreads();
    int count = 0;   // matched keypoints of the frame, the same in every lane after the loop
    for (int base = 0; base < n; base += PAIRS_THREADS) {   // n is uniform: every lane takes every turn
        const int k = base + tid;
        const int mc = k < n ? match_cand[k0 + k] : -1;
        const bool on = mc >= 0 && mc < nc;   // (a candidate index outside the frame cannot be looked up: no pair)
        const int key = on ? kp_lmid[k0 + k] : 0;
        int rank = 0;
        for (int cb = 0; cb < n; cb += PAIRS_THREADS) {
            const int q = cb + tid;
            const int mq = q < n ? match_cand[k0 + q] : -1;
            __syncthreads();
            s_on[tid] = mq >= 0 && mq < nc;
            s_key[tid] = s_on[tid] ? kp_lmid[k0 + q] : 0;
            __syncthreads();
            if (!on) continue;
            const int m = min(PAIRS_THREADS, n - cb);
            for (int t = 0; t < m; ++t)
                rank += s_on[t] && (s_key[t] < key || (s_key[t] == key && cb + t < k));
        }
        if (on) {
            prev_lmid[k0 + rank] = key;
            new_lmid[k0 + rank] = cand_lmid[c0 + mc];
        }
        const unsigned long long bal = __ballot(on);
        if ((tid & 63) == 0 && bal) atomicAdd(&s_count, __popcll(bal));
    }
    __syncthreads();
    count = s_count;
    for (int t = count + tid; t < n; t += PAIRS_THREADS) { prev_lmid[k0 + t] = -1; new_lmid[k0 + t] = -1; }
    if (tid == 0) n_pairs[b] = count;
}

}  // namespace

extern "C" ov2_status ov2_match_pairs_dev(ov2_ctx *c, int B, int n_kp, const int32_t *d_kp_off, const int32_t *d_cand_off,
                                          const int32_t *d_kp_lmid, const int32_t *d_cand_lmid, const int32_t *d_match_cand,
                                          int32_t *d_prev_lmid, int32_t *d_new_lmid, int32_t *d_n_pairs)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || n_kp < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_match_pairs_dev: negative count");
    if (B == 0) return OV2_OK;
    if (!d_kp_off || !d_cand_off || !d_n_pairs || (n_kp && (!d_kp_lmid || !d_cand_lmid || !d_match_cand || !d_prev_lmid || !d_new_lmid)))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_match_pairs_dev: null argument");
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_LAUNCH(c, K_MATCH, match_pairs_kernel, dim3(B), dim3(PAIRS_THREADS), 0, c->stream, d_kp_off, d_cand_off, d_kp_lmid, d_cand_lmid,
               d_match_cand, d_prev_lmid, d_new_lmid, d_n_pairs);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}
