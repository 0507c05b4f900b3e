// fastnms.hip -- whole-image FAST-9/16 with 3x3 non-maximum suppression, a byte mask and retainBest, batched, on gfx950.
//
// Replaces the detector half of the reference's LoopCloser::run, src/loop_closer.cpp:95-126: the mask with a
// cv::circle(mask, kp.px_, 2, 0, FILLED) per described keypoint (:95-109), cv::FastFeatureDetector(20)->detect(img, kps, mask)
// (:123; OpenCV's FAST_t<16> with nonmaxSuppression, then KeyPointsFilter::runByPixelsMask) and
// cv::KeyPointsFilter::retainBest(kps, 300) (:126).  Everything is integer arithmetic, so the result is exact.
//
// Launches (their number depends neither on the batch nor on the number of keypoints):
//   fast_mask_kernel    discs of the mask points into a zeroed byte plane (eight lanes per point), skipped without a mask
//   fast_score_kernel   a workgroup per 64 x 16 tile: tile + 3-pixel ring staged in LDS as dwords, four scores per thread,
//                       one dword store into the byte score plane (0 outside 3 <= x < w-3, 3 <= y < h-3)
//   fast_nms_kernel     a wave per image row, 4 or 16 rows per workgroup: strict 3x3 maximum, then the mask; survivors keep their
//                       score in the keypoint plane, and a 256-bin histogram of their responses is summed per image
//   fast_count_kernel   the same shape: the response bound r* of retainBest from the histogram (once per workgroup), survivors
//                       >= r* per row
//   fast_emit_kernel    the same shape: rows above summed, then an ordered compaction of the row (scan over the wave, then writes)
// The output order is row-major (y, then x ascending) and identical from run to run: the only atomics are integer counts.
#include "ov2_internal.h"
#include "ov2_detect.h"

#include <algorithm>

namespace {

enum { K_FAST_SCORE = OV2_K_MAP + 19, K_FAST_NMS = OV2_K_MAP + 20, K_FAST_SELECT = OV2_K_MAP + 21 };

#define FD_TW 64               // tile of the score pass, pixels
#define FD_TH 16
#define FD_LW (FD_TW + 8)      // staged bytes per row: x0 - 4 .. x0 + 67 (whole dwords; the ring needs x0 - 3 .. x0 + 66)
#define FD_LH (FD_TH + 6)      // staged rows: y0 - 3 .. y0 + 18
// rows per workgroup of the suppression, count and emit passes (a wave per row, a wave takes every fourth row): a few images
// want many short workgroups, a large batch wants the per-workgroup set-up (histogram, retainBest bound) spread over more rows
#define FD_ROWS_FEW 4
#define FD_ROWS_MANY 16
#define FD_ROWS_MANY_FROM 8192   // image rows in the call from which FD_ROWS_MANY is used
#define FD_MASK_LANES 8
#define FD_MASK_PTS (256 / FD_MASK_LANES)

// discs of the mask points: lane j of a point's group walks the spans of disc rows j, j + 8, ...; every store writes 1
__global__ __launch_bounds__(256) void fast_mask_kernel(const float2 *__restrict__ pts, const int *__restrict__ pt_img, int n, int B,
                                                        unsigned char *__restrict__ mask_all, int w, int h, int sp, disc_shape ds)
{
    const int sub = threadIdx.x % FD_MASK_LANES;
    for (int k = blockIdx.x * FD_MASK_PTS + threadIdx.x / FD_MASK_LANES; k < n; k += gridDim.x * FD_MASK_PTS) {
        const float2 p = pts[k];
        const int b = pt_img[k];
        if (b < 0 || b >= B) continue;
        // cv::Point2f -> cv::Point: cvRound, half to even
        const float fx = __builtin_rintf(p.x), fy = __builtin_rintf(p.y);
        if (!(fx >= (float)-ds.r && fx < (float)(w + ds.r) && fy >= (float)-ds.r && fy < (float)(h + ds.r))) continue;   // no pixel inside (or NaN)
        const int cx = (int)fx, cy = (int)fy;
        unsigned char *mask = mask_all + (size_t)b * sp * h;
        for (int row = sub; row <= 2 * ds.r; row += FD_MASK_LANES) {
            const int hw = ds.hw[row], y = cy + row - ds.r;
            if (hw < 0 || y < 0 || y >= h) continue;
            const int xa = max(cx - hw, 0), xb = min(cx + hw, w - 1);
            for (int x = xa; x <= xb; ++x) mask[(size_t)y * sp + x] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void fast_score_kernel(const unsigned char *__restrict__ img0, size_t img_bstride, int istride,
                                                         int w, int h, int threshold, unsigned char *__restrict__ score_all, int sp)
{
    __shared__ unsigned tile[FD_LH * (FD_LW / 4)];
    const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * FD_TW, y0 = blockIdx.y * FD_TH;
    const unsigned char *img = img0 + img_bstride * b;
    // only pixels of the image are loaded (whole aligned dwords of its rows); what lies outside is never part of a ring
    for (int i = tid; i < FD_LH * (FD_LW / 4); i += 256) {
        const int ly = i / (FD_LW / 4), lq = i - ly * (FD_LW / 4);
        const int y = y0 - 3 + ly, x = x0 - 4 + 4 * lq;
        unsigned v = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) v = *reinterpret_cast<const unsigned *>(img + (size_t)y * istride + x);
        tile[i] = v;
    }
    __syncthreads();
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(tile);
    const int ry = tid / (FD_TW / 4), xq = tid - ry * (FD_TW / 4);
    const int y = y0 + ry, xb = x0 + 4 * xq;
    if (y >= h || xb >= sp) return;
    unsigned out = 0;
    if (y >= 3 && y < h - 3) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xb + k;
            if (x >= 3 && x < w - 3) out |= (unsigned)fast_score(tb + (ry + 3) * FD_LW + 4 + 4 * xq + k, FD_LW, threshold) << (8 * k);
        }
    }
    *reinterpret_cast<unsigned *>(score_all + ((size_t)b * h + y) * sp + xb) = out;
}

// bytes x-1 .. x+4 of a plane row around dword q (x = 4 q) in bits 0 .. 47; beyond the row: 0
__device__ __forceinline__ unsigned long long row_window(const unsigned *__restrict__ r, int q, int nq)
{
    if (!r) return 0ull;
    unsigned long long v = (unsigned long long)r[q] << 8;
    if (q > 0) v |= r[q - 1] >> 24;
    if (q + 1 < nq) v |= (unsigned long long)(r[q + 1] & 0xffu) << 40;
    return v;
}

__global__ __launch_bounds__(256) void fast_nms_kernel(const unsigned char *__restrict__ score_all, const unsigned char *__restrict__ mask_all,
                                                       int h, int sp, int rows, unsigned char *__restrict__ kp_all, unsigned *__restrict__ hist_all)
{
    __shared__ unsigned lh[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, nq = sp / 4;
    lh[tid] = 0;
    __syncthreads();
    for (int ry = wv; ry < rows; ry += 4) {   // a wave per row
        const int y = blockIdx.x * rows + ry;
        if (y >= h) break;
        const size_t row = ((size_t)b * h + y) * sp;
        const unsigned *r1 = reinterpret_cast<const unsigned *>(score_all + row);
        const unsigned *r0 = y > 0 ? r1 - nq : nullptr, *r2 = y < h - 1 ? r1 + nq : nullptr;
        const unsigned *mk = mask_all ? reinterpret_cast<const unsigned *>(mask_all + row) : nullptr;
        unsigned *kp = reinterpret_cast<unsigned *>(kp_all + row);
        for (int q = lane; q < nq; q += 64) {
            unsigned out = 0;
            if (r1[q]) {
                const unsigned long long a = row_window(r0, q, nq), m = row_window(r1, q, nq), d = row_window(r2, q, nq);
                const unsigned masked = mk ? mk[q] : 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned s = (unsigned)(m >> (8 * (k + 1))) & 0xffu;
                    if (!s) continue;
                    const unsigned a3 = (unsigned)(a >> (8 * k)), d3 = (unsigned)(d >> (8 * k)), m3 = (unsigned)(m >> (8 * k));
                    unsigned mx = max(max(a3 & 0xffu, (a3 >> 8) & 0xffu), (a3 >> 16) & 0xffu);
                    mx = max(mx, max(max(d3 & 0xffu, (d3 >> 8) & 0xffu), (d3 >> 16) & 0xffu));
                    mx = max(mx, max(m3 & 0xffu, (m3 >> 16) & 0xffu));
                    if (s > mx && !((masked >> (8 * k)) & 0xffu)) {   // the mask comes after the suppression (runByPixelsMask)
                        out |= s << (8 * k);
                        atomicAdd(&lh[s], 1u);
                    }
                }
            }
            kp[q] = out;
        }
    }
    __syncthreads();
    if (lh[tid]) atomicAdd(&hist_all[(size_t)b * 256 + tid], lh[tid]);
}

// KeyPointsFilter::retainBest(n_best) on byte responses: the smallest response kept (256 = none) and the number kept.
// hist[t] = keypoints of response t; sh: 256 words; all 256 threads call it.
__device__ __forceinline__ int retain_bound(const unsigned *__restrict__ hist, int n_best, unsigned *sh, int *kept)
{
    __shared__ int bound, nkept;
    const int t = threadIdx.x;
    sh[t] = t ? hist[t] : 0u;   // a keypoint has a response > 0
    if (t == 0) { bound = 256; nkept = 0; }
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {   // suffix sums: sh[t] = keypoints of response >= t
        const unsigned v = t + o < 256 ? sh[t + o] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    const unsigned total = sh[0], mine = sh[t], above = t < 255 ? sh[t + 1] : 0u;
    if (n_best < 0 || total <= (unsigned)n_best) {
        if (t == 1) { bound = 1; nkept = (int)total; }
    } else if (n_best > 0 && t >= 1 && mine >= (unsigned)n_best && above < (unsigned)n_best) {   // the n_best-th largest response
        bound = t; nkept = (int)mine;
    }
    __syncthreads();
    *kept = nkept;
    return bound;
}

// number of bytes >= bound (1 .. 256) in a dword
__device__ __forceinline__ int count_ge(unsigned v, unsigned bound)
{
    return (int)((v & 0xffu) >= bound) + (int)(((v >> 8) & 0xffu) >= bound) + (int)(((v >> 16) & 0xffu) >= bound) + (int)((v >> 24) >= bound);
}

// sum over the wave, known to all its lanes
__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void fast_count_kernel(const unsigned char *__restrict__ kp_all, const unsigned *__restrict__ hist_all,
                                                         int h, int sp, int rows, int n_best, int *__restrict__ rowcnt_all)
{
    __shared__ unsigned sh[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, nq = sp / 4;
    int kept;
    const unsigned bound = (unsigned)retain_bound(hist_all + (size_t)b * 256, n_best, sh, &kept);
    for (int ry = wv; ry < rows; ry += 4) {   // a wave per row
        const int y = blockIdx.x * rows + ry;
        if (y >= h) break;
        const unsigned *kp = reinterpret_cast<const unsigned *>(kp_all + ((size_t)b * h + y) * sp);
        int n = 0;
        if (kept > 0)
            for (int q = lane; q < nq; q += 64) n += count_ge(kp[q], bound);
        n = wave_sum(n);
        if (lane == 0) rowcnt_all[(size_t)b * h + y] = n;
    }
}

__global__ __launch_bounds__(256) void fast_emit_kernel(const unsigned char *__restrict__ kp_all, const unsigned *__restrict__ hist_all,
                                                        const int *__restrict__ rowcnt_all, int h, int sp, int rows, int n_best, int out_cap,
                                                        int *__restrict__ n_total, int *__restrict__ n_out, float2 *__restrict__ out_xy,
                                                        unsigned char *__restrict__ out_resp)
{
    __shared__ unsigned sh[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, nq = sp / 4;
    int kept;
    const unsigned bound = (unsigned)retain_bound(hist_all + (size_t)b * 256, n_best, sh, &kept);
    if (blockIdx.x == 0 && tid == 0) { n_total[b] = kept; n_out[b] = min(kept, out_cap); }
    if (kept == 0) return;
    const int *rowcnt = rowcnt_all + (size_t)b * h;
    float2 *o = out_xy + (size_t)b * out_cap;
    unsigned char *oresp = out_resp + (size_t)b * out_cap;
    for (int ry = wv; ry < rows; ry += 4) {   // a wave per row; everything below is uniform over the wave
        const int y = blockIdx.x * rows + ry;
        if (y >= h) break;
        if (rowcnt[y] == 0) continue;
        int above = 0;
        for (int r = lane; r < y; r += 64) above += rowcnt[r];
        int base = wave_sum(above);   // keypoints of the rows above: this row's first place in the list
        if (base >= out_cap) break;   // and the rows below start even later
        const unsigned *kp = reinterpret_cast<const unsigned *>(kp_all + ((size_t)b * h + y) * sp);
        for (int q0 = 0; q0 < nq; q0 += 64) {   // ordered compaction: counts, a scan over the wave, then the writes
            const int q = q0 + lane;
            const unsigned v = q < nq ? kp[q] : 0u;
            const int c = count_ge(v, bound);
            int inc = c;
            for (int s = 1; s < 64; s <<= 1) {
                const int t = __shfl_up(inc, s);
                if (lane >= s) inc += t;
            }
            int pos = base + inc - c;
            base += __shfl(inc, 63);
            if (c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned s = (v >> (8 * k)) & 0xffu;
                    if (s >= bound) {
                        if (pos < out_cap) { o[pos] = make_float2((float)(4 * q + k), (float)y); oresp[pos] = (unsigned char)s; }
                        ++pos;
                    }
                }
            }
        }
    }
}

}  // namespace

// Everything on the device, nothing synchronous.  Scratch: [histograms | mask plane] zeroed by one fill, then the score plane,
// the keypoint plane and the per-row counts; the planes have a pitch of whole dwords.
extern "C" ov2_status ov2_fast_detect_batch_dev(ov2_ctx *c, const ov2_pyr *pyr, int threshold, int mask_radius, int n_mask,
                                                const float *d_mask_xy, const int32_t *d_mask_img, int n_best, int out_cap,
                                                int32_t *d_n_total, int32_t *d_n_out, float *d_out_xy, uint8_t *d_out_resp)
{
    if (!c) return OV2_ERR_INVALID;
    if (!pyr || !d_n_total || !d_n_out) return ov2_set_err(c, OV2_ERR_INVALID, "null argument");
    if (out_cap < 0 || (out_cap > 0 && (!d_out_xy || !d_out_resp))) return ov2_set_err(c, OV2_ERR_INVALID, "out_cap %d / null output arrays", out_cap);
    if (mask_radius > DET_MAX_R) return ov2_set_err(c, OV2_ERR_INVALID, "mask radius %d above %d", mask_radius, DET_MAX_R);
    if (n_mask < 0 || (n_mask > 0 && mask_radius >= 0 && (!d_mask_xy || !d_mask_img))) return ov2_set_err(c, OV2_ERR_INVALID, "mask points");
    OV2_HIP(c, hipSetDevice(c->device));
    {
        const ov2_status ws = ov2_pyr_wait_ready(c, pyr);
        if (ws != OV2_OK) return ws;
    }
    const ov2_pyr_view &v = pyr->buf->view;
    const ov2_level_desc &L = v.lv[0];
    const int B = pyr->buf->batch, w = L.w, h = L.h;
    if (B <= 0 || B > 65535 || w <= 0 || h <= 0) return ov2_set_err(c, OV2_ERR_INVALID, "batch %d of %d x %d images", B, w, h);
    const unsigned char *img = v.base + L.img_off + (size_t)v.pad * L.istride + OV2_LM;
    const int sp = ov2_round_up(w, 4);
    const bool use_mask = mask_radius >= 0 && n_mask > 0;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t plane = up((size_t)sp * h * B);
    const size_t off_hist = 0, off_mask = up(sizeof(unsigned) * 256 * (size_t)B), zero_bytes = off_mask + (use_mask ? plane : 0);
    const size_t off_score = zero_bytes, off_kp = off_score + plane, off_rows = off_kp + plane;
    const size_t total = off_rows + up(sizeof(int) * (size_t)h * B);
    void *scr = nullptr;
    const ov2_status s = ov2_scratch(c, total, &scr);
    if (s != OV2_OK) return s;
    hipStream_t st = c->stream;
    char *base = (char *)scr;
    unsigned *hist = (unsigned *)(base + off_hist);
    unsigned char *mask = use_mask ? (unsigned char *)(base + off_mask) : nullptr;
    unsigned char *score = (unsigned char *)(base + off_score), *kp = (unsigned char *)(base + off_kp);
    int *rowcnt = (int *)(base + off_rows);
    const int rows = (size_t)h * B >= FD_ROWS_MANY_FROM ? FD_ROWS_MANY : FD_ROWS_FEW;
    OV2_HIP(c, hipMemsetAsync(base, 0, zero_bytes, st));
    if (use_mask)
        OV2_LAUNCH_ON(c, K_FAST_SELECT, st, fast_mask_kernel, dim3(std::min((n_mask + FD_MASK_PTS - 1) / FD_MASK_PTS, 65536)), dim3(256), 0, st,
                      reinterpret_cast<const float2 *>(d_mask_xy), d_mask_img, n_mask, B, mask, w, h, sp, make_disc(mask_radius));
    OV2_LAUNCH_ON(c, K_FAST_SCORE, st, fast_score_kernel, dim3((sp + FD_TW - 1) / FD_TW, (h + FD_TH - 1) / FD_TH, B), dim3(256), 0, st, img,
                  L.img_bstride, L.istride, w, h, std::min(std::max(threshold, 0), 255), score, sp);
    OV2_LAUNCH_ON(c, K_FAST_NMS, st, fast_nms_kernel, dim3((h + rows - 1) / rows, B), dim3(256), 0, st, score, mask, h, sp, rows, kp, hist);
    OV2_LAUNCH_ON(c, K_FAST_SELECT, st, fast_count_kernel, dim3((h + rows - 1) / rows, B), dim3(256), 0, st, kp, hist, h, sp, rows, n_best, rowcnt);
    OV2_LAUNCH_ON(c, K_FAST_SELECT, st, fast_emit_kernel, dim3((h + rows - 1) / rows, B), dim3(256), 0, st, kp, hist, rowcnt, h, sp, rows, n_best, out_cap, d_n_total,
                  d_n_out, reinterpret_cast<float2 *>(d_out_xy), d_out_resp);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

// host-pointer form: stages the arguments through pinned memory, runs the device pipeline, one synchronisation
extern "C" ov2_status ov2_fast_detect_batch(ov2_ctx *c, const ov2_pyr *pyr, int threshold, int mask_radius, const int *n_mask,
                                            const float *mask_xy, int n_best, int out_cap, int *n_total, int *n_out, float *out_xy,
                                            uint8_t *out_resp)
{
    if (!c) return OV2_ERR_INVALID;
    if (!pyr || !n_total || !n_out) return ov2_set_err(c, OV2_ERR_INVALID, "null argument");
    if (out_cap < 0 || (out_cap > 0 && (!out_xy || !out_resp))) return ov2_set_err(c, OV2_ERR_INVALID, "out_cap %d / null output arrays", out_cap);
    if (mask_radius > DET_MAX_R) return ov2_set_err(c, OV2_ERR_INVALID, "mask radius %d above %d", mask_radius, DET_MAX_R);
    const int B = pyr->buf->batch;
    int nm = 0;
    if (mask_radius >= 0 && n_mask) {
        for (int b = 0; b < B; ++b) {
            if (n_mask[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative mask point count");
            nm += n_mask[b];
        }
        if (nm && !mask_xy) return ov2_set_err(c, OV2_ERR_INVALID, "null mask_xy");
    }
    OV2_HIP(c, hipSetDevice(c->device));
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // pinned staging (host) and its device twin: [mask_img | mask_xy | n_total B | n_out B | out_xy B x cap | out_resp B x cap]
    const size_t o_mi = 0, o_mx = up(sizeof(int) * (size_t)nm), o_nt = o_mx + up(8 * (size_t)nm), o_no = o_nt + up(sizeof(int) * B);
    const size_t o_ox = o_no + up(sizeof(int) * B), o_or = o_ox + up(8 * (size_t)B * out_cap), total = o_or + up((size_t)B * out_cap);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    hipStream_t st = c->stream;
    if (nm) {
        int *mi = (int *)(hp + o_mi);
        int k = 0;
        for (int b = 0; b < B; ++b)
            for (int q = 0; q < n_mask[b]; ++q) mi[k++] = b;
        memcpy(hp + o_mx, mask_xy, 8 * (size_t)nm);
        OV2_HIP(c, hipMemcpyAsync(dp, hp, o_nt, hipMemcpyHostToDevice, st));
    }
    s = ov2_fast_detect_batch_dev(c, pyr, threshold, mask_radius, nm, (const float *)(dp + o_mx), (const int32_t *)(dp + o_mi), n_best, out_cap,
                                  (int32_t *)(dp + o_nt), (int32_t *)(dp + o_no), (float *)(dp + o_ox), (uint8_t *)(dp + o_or));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_nt, dp + o_nt, total - o_nt, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(n_total, hp + o_nt, sizeof(int) * B);
    memcpy(n_out, hp + o_no, sizeof(int) * B);
    for (int b = 0; b < B; ++b)
        if (n_out[b] > 0) {
            memcpy(out_xy + (size_t)b * out_cap * 2, hp + o_ox + 8 * (size_t)b * out_cap, 8 * (size_t)n_out[b]);
            memcpy(out_resp + (size_t)b * out_cap, hp + o_or + (size_t)b * out_cap, (size_t)n_out[b]);
        }
    return OV2_OK;
}
