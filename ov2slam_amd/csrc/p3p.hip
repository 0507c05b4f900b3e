// p3p.hip -- the P3P stage of computePose on gfx950: batched P3P LMedS / RANSAC (f64).
//
// Replaces (reference): MultiViewGeometry::p3pRansac src/multi_view_geometry.cpp:144-163 -> opengvP3PLMeds :257-343
// (use_lmeds, what VisualFrontEnd::computePose calls, src/visual_front_end.cpp:718-782) and opengvP3PRansac :168-254
// (what the loop closer calls).  OpenGV is an un-vendored dependency; what is restated here is its published source
// (sac/Lmeds.hpp, sac/Ransac.hpp, AbsolutePoseSacProblem with KNEIP) and Kneip's paper (CVPR 2011):
//   * model of a draw of 4 correspondences: Kneip's P3P on the first three (p3p_model.h), the fourth picks the solution
//     with the lowest 1 - f4 . p / |p|; no real solution -> the draw is skipped;
//   * distance of correspondence i: 1 - f_i . p_i / |p_i|, p_i = R^T (X_i - t); th = 1 - cos(atan(errth / focal));
//   * Lmeds::computeModel: while (iterations < max_iter && skipped < 10 max_iter) { draw; no model -> ++skipped,
//     continue; sort the n distances; penalty = sqrt(d[n/2]) (odd n) or (sqrt(d[n/2-1]) + sqrt(d[n/2])) / 2; penalty <
//     best (best starts at DBL_MAX) -> new best; ++iterations }.  Inliers: d_i <= th under the best model.
//   * Ransac::computeModel, probability 0.99, sample size 4: as epipolar.hip states it for sample size 5; inliers d_i < th.
// Deviations (parity section): the sampler (sac_common.h; the reference seeds OpenGV from the clock); a
// distance is clamped below at 0 and a non-finite one (NaN bearing or point, point at the camera centre) counts as
// +infinity (sorts last, never an inlier; a ZERO bearing has the finite distance 1: above any threshold, not last); only real
// roots of Kneip's quartic give candidates, and the candidates are polished (p3p_model.h).
//
// Mapping: LMedS has no early exit, so all hypotheses are independent.  A call is a chain of four launches per block
// of draws; the per-frame state is carried in the workspace from one block to the next.  The first block holds
// 2 min(nmaxiter, 256) + 32 draws, enough unless more than half of them have no model; the later ones (up to
// 11 min(nmaxiter, 256) + 1 draws each, one of them for nmaxiter <= 256) cover the skip budget and retire at once for
// a frame that is done:
//   1. p3p_solve_kernel   one LANE per (frame, draw): sampler, Kneip, 4th-point pick -> model + valid flag
//   2. p3p_select_kernel  one workgroup per frame: prefix count of the valid draws -> the list of counted draws
//                         (the first max_iter valid ones within the skip budget)
//   3. p3p_score_kernel   one workgroup per (frame, counted draw): the n distances (kept in LDS up to 4096 of them,
//                         recomputed beyond), then the exact order statistics n/2 - 1 and n/2 by an 8-pass radix
//                         select on the 64-bit patterns (non-negative doubles order like their bit patterns) -> penalty;
//                         in RANSAC mode the count of d < th instead
//   4. p3p_final_kernel   one workgroup per frame: first draw of the lowest penalty (= the sequential strict-< rule),
//                         or OpenGV's RANSAC loop replayed over the counts in draw order; on the last block the
//                         classification, the status rule and R -> quaternion.
// Every loop bound depends on n and nmaxiter only.  Nothing is synchronised or read back by the _dev form.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ov2_internal.h"
#include "ov2_se3.h"

#define HD __host__ __device__
#include "p3p_model.h"

namespace {

enum { P3P_THREADS = 256, P3P_LDS_N = 4096, P3P_MAX_BLOCK_ITER = 256,
       K_P3P_SOLVE = OV2_K_MAP + 9, K_P3P_SELECT = OV2_K_MAP + 10, K_P3P_SCORE = OV2_K_MAP + 11, K_P3P_FINAL = OV2_K_MAP + 12,
       K_P3P_DBG = OV2_K_MAP + 13 };

// per-frame state carried from one block of draws to the next
struct p3p_state {
    double best_pen, k, best[12];    // best_pen: LMedS; k (OpenGV's iteration bound) and best_cnt: RANSAC
    int counted, skipped, done, best_d, best_cnt, ncnt, skip0, pad;   // skip0: skipped before this block
};

struct p3p_args {
    int nmaxiter, mode, D, L;        // mode 0 = LMedS, 1 = RANSAC; D draws per block; L = list capacity per block
    int d0, first, last;             // first draw of this block
    float errth;
    const int32_t *off;
    const double *bv, *X, *K;
    const uint64_t *seed;
    double *Twc;
    uint8_t *outlier;
    int32_t *status, *info;
    // workspace
    double *model;                   // B x D x 12
    int32_t *valid;                  // B x D
    int32_t *list;                   // B x L   draw (relative to d0) of the k-th counted one of this block
    double *pen;                     // B x L   penalty (LMedS) / count as a double (RANSAC)
    p3p_state *st;                   // B
};

__global__ __launch_bounds__(P3P_THREADS) void p3p_solve_kernel(p3p_args A)
{
    __shared__ p3p_ws W[P3P_THREADS];
    const int b = blockIdx.y, dl = blockIdx.x * P3P_THREADS + threadIdx.x;
    if (dl >= A.D) return;
    const int o0 = A.off[b], n = A.off[b + 1] - o0;
    const size_t slot = (size_t)b * A.D + dl;
    if (n < 4 || (!A.first && A.st[b].done)) { A.valid[slot] = 0; return; }
    int idx[4];
    sac_draw<4>(A.seed[b], A.d0 + dl, n, idx);
    double f[4][3], X[4][3], m[12];
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < 3; ++k) {
            f[s][k] = A.bv[3 * (size_t)(o0 + idx[s]) + k];
            X[s][k] = A.X[3 * (size_t)(o0 + idx[s]) + k];
        }
    const bool ok = p3p_model(f, X, W[threadIdx.x], m);
    A.valid[slot] = ok;
    if (ok)
        for (int e = 0; e < 12; ++e) A.model[12 * slot + e] = m[e];
}

// exclusive block scan of one int per thread (256 threads); every thread gets its prefix, *total the sum
__device__ inline int block_scan(int v, int *sh, int *total)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < P3P_THREADS; o <<= 1) {
        const int x = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    const int incl = sh[tid];
    *total = sh[P3P_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(P3P_THREADS) void p3p_select_kernel(p3p_args A)
{
    __shared__ int sh[P3P_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o0 = A.off[b], n = A.off[b + 1] - o0;
    p3p_state &S = A.st[b];
    if (A.first) {
        __syncthreads();
        if (tid == 0) {
            S.best_pen = DBL_MAX; S.k = 1.0; S.counted = 0; S.skipped = 0; S.best_d = -1; S.best_cnt = -INT_MAX; S.ncnt = 0;
            S.done = n < 4 || A.nmaxiter <= 0;   // the loops' first test: 0 < max_iter (LMedS), 0 < 10 max_iter (RANSAC)
        }
        __syncthreads();
    }
    const int done0 = S.done, counted0 = S.counted, skipped0 = S.skipped;
    __syncthreads();
    if (done0) {
        if (tid == 0) S.ncnt = 0;
        return;
    }
    // a draw is looked at iff the counts of valid / invalid draws before it are below their limits (both are monotone)
    const int lim = A.mode == 0 ? A.nmaxiter : A.nmaxiter + 1, max_skip = 10 * A.nmaxiter;
    const int per = (A.D + P3P_THREADS - 1) / P3P_THREADS, j0 = tid * per, j1 = min(A.D, j0 + per);
    const int32_t *valid = A.valid + (size_t)b * A.D;
    int nv = 0;
    for (int j = j0; j < j1; ++j) nv += valid[j] != 0;
    int tot;
    int pv = block_scan(nv, sh, &tot);
    int cv = counted0 + pv, ci = skipped0 + (j0 < A.D ? j0 : A.D) - pv;   // valid / invalid before draw j
    int mine = 0, skip_mine = 0, stop = 0;
    for (int j = j0; j < j1; ++j) {
        const bool look = cv < lim && ci < max_skip;
        if (!look) stop = 1;
        if (valid[j]) {
            if (look) { A.list[(size_t)b * A.L + (cv - counted0)] = j; ++mine; }
            ++cv;
        } else {
            if (look) ++skip_mine;
            ++ci;
        }
    }
    int t1, t2, t3;
    block_scan(mine, sh, &t1);
    block_scan(skip_mine, sh, &t2);
    block_scan(stop, sh, &t3);
    if (tid == 0) {
        S.ncnt = t1;
        S.skip0 = skipped0;
        S.skipped = skipped0 + t2;
        // LMedS counts here; RANSAC counts its iterations in the replay (the bound k may end it sooner)
        if (A.mode == 0) S.counted = counted0 + t1;
        if (t3 || !(counted0 + t1 < lim && skipped0 + t2 < max_skip)) S.done = 1;
    }
}

__device__ inline double p3p_point_dist(const p3p_args &A, const double *m, int g)
{
    const double f[3] = {A.bv[3 * (size_t)g], A.bv[3 * (size_t)g + 1], A.bv[3 * (size_t)g + 2]};
    const double X[3] = {A.X[3 * (size_t)g], A.X[3 * (size_t)g + 1], A.X[3 * (size_t)g + 2]};
    return p3p_dist(m, m + 9, f, X);
}

__global__ __launch_bounds__(P3P_THREADS) void p3p_score_kernel(p3p_args A)
{
    __shared__ double dsh[P3P_LDS_N];
    __shared__ int hist[P3P_THREADS], sh[P3P_THREADS];
    __shared__ unsigned long long s_prefix, s_red[P3P_THREADS / 64];
    __shared__ int s_rank;
    const int b = blockIdx.y, kk = blockIdx.x, tid = threadIdx.x;
    if (kk >= A.st[b].ncnt) return;
    const int o0 = A.off[b], n = A.off[b + 1] - o0;
    const int dl = A.list[(size_t)b * A.L + kk];
    double m[12];
    for (int e = 0; e < 12; ++e) m[e] = A.model[12 * ((size_t)b * A.D + dl) + e];
    if (A.mode == 1) {   // RANSAC: the count of distances below the threshold
        const double th = p3p_threshold(A.K[4 * b], A.K[4 * b + 1], A.errth);
        int c = 0;
        for (int i = tid; i < n; i += P3P_THREADS) c += p3p_point_dist(A, m, o0 + i) < th;
        int tot;
        block_scan(c, sh, &tot);
        if (tid == 0) A.pen[(size_t)b * A.L + kk] = (double)tot;
        return;
    }
    for (int i = tid; i < n && i < P3P_LDS_N; i += P3P_THREADS) dsh[i] = p3p_point_dist(A, m, o0 + i);
    if (tid == 0) { s_prefix = 0ull; s_rank = n / 2; }
    __syncthreads();
    auto key = [&](int i) -> unsigned long long {
        return (unsigned long long)__double_as_longlong(i < P3P_LDS_N ? dsh[i] : p3p_point_dist(A, m, o0 + i));
    };
    // radix select of rank n / 2, most significant byte first
    for (int pass = 7; pass >= 0; --pass) {
        hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const int shift = 8 * pass;
        for (int i = tid; i < n; i += P3P_THREADS) {
            const unsigned long long k = key(i);
            if (pass == 7 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((k >> shift) & 255ull)], 1);
        }
        __syncthreads();
        const int h = hist[tid], rank = s_rank;
        int tot;
        const int ex = block_scan(h, sh, &tot);
        if (rank >= ex && rank < ex + h) {
            s_prefix = prefix | ((unsigned long long)tid << shift);
            s_rank = rank - ex;
        }
        __syncthreads();
    }
    const unsigned long long kmid = s_prefix;
    const int r_in_bucket = s_rank;   // rank of d[n/2] among the keys equal to it: n/2 - #(keys below)
    double dmid = __longlong_as_double((long long)kmid), dlow = dmid;
    if ((n & 1) == 0 && r_in_bucket == 0) {   // d[n/2 - 1] is the largest key below d[n/2]
        unsigned long long best = 0ull;
        for (int i = tid; i < n; i += P3P_THREADS) {
            const unsigned long long k = key(i);
            if (k < kmid && k > best) best = k;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long x = __shfl_xor(best, o);
            best = x > best ? x : best;
        }
        if ((tid & 63) == 0) s_red[tid >> 6] = best;
        __syncthreads();
        for (int w = 0; w < P3P_THREADS / 64; ++w) best = s_red[w] > best ? s_red[w] : best;
        dlow = __longlong_as_double((long long)best);
    }
    if (tid == 0)
        A.pen[(size_t)b * A.L + kk] = (n & 1) ? p3p_sqrt(dmid) : (p3p_sqrt(dlow) + p3p_sqrt(dmid)) / 2.;
}

__global__ __launch_bounds__(P3P_THREADS) void p3p_final_kernel(p3p_args A)
{
    __shared__ int sh[P3P_THREADS];
    __shared__ double s_pen[P3P_THREADS / 64];
    __shared__ int s_idx[P3P_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o0 = A.off[b], n = A.off[b + 1] - o0;
    p3p_state &S = A.st[b];
    const int ncnt = S.ncnt;
    const double *pen = A.pen + (size_t)b * A.L;
    const int32_t *list = A.list + (size_t)b * A.L;
    if (A.mode == 0) {
        // the first counted draw of the lowest penalty; a block's winner replaces the carried best only if strictly lower
        double bp = INFINITY;
        int bi = INT_MAX;
        for (int k = tid; k < ncnt; k += P3P_THREADS) {
            const double p = pen[k];
            if (p < bp) { bp = p; bi = k; }   // k ascending per thread: the first of equals stays
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double p = __shfl_xor(bp, o);
            const int i = __shfl_xor(bi, o);
            if (p < bp || (p == bp && i < bi)) { bp = p; bi = i; }
        }
        if ((tid & 63) == 0) { s_pen[tid >> 6] = bp; s_idx[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < P3P_THREADS / 64; ++w)
                if (s_pen[w] < bp || (s_pen[w] == bp && s_idx[w] < bi)) { bp = s_pen[w]; bi = s_idx[w]; }
            if (bi != INT_MAX && bp < S.best_pen) {
                S.best_pen = bp;
                S.best_d = A.d0 + list[bi];
                for (int e = 0; e < 12; ++e) S.best[e] = A.model[12 * ((size_t)b * A.D + list[bi]) + e];
            }
        }
    } else if (tid == 0) {
        // OpenGV's RANSAC loop over this block's counted draws, in draw order (skipped draws were budgeted by the
        // select kernel; a handful of integer compares per draw, the classification below is the kernel's work)
        int it = S.counted, lastk = -1;
        bool stop = false;
        for (int k = 0; k < ncnt && !stop; ++k) {
            if (!((double)it < S.k)) { stop = true; break; }
            const int c = (int)pen[k];
            if (c > S.best_cnt) {
                S.best_cnt = c;
                S.best_d = A.d0 + list[k];
                for (int e = 0; e < 12; ++e) S.best[e] = A.model[12 * ((size_t)b * A.D + list[k]) + e];
                S.k = sac_ransac_k(c, n, 4.0);
            }
            ++it;
            lastk = k;
            if (it > A.nmaxiter) stop = true;
        }
        S.counted = it;
        stop = stop || !((double)it < S.k);
        // the loop ended behind counted draw lastk: the invalid draws after it were never looked at
        if (stop && lastk >= 0) S.skipped = S.skip0 + list[lastk] - lastk;
        if (stop) S.done = 1;
    }
    __syncthreads();
    if (!A.last) return;
    // classification under the best model, the return rule, R -> quaternion
    const int best_d = S.best_d;
    double m[12];
    for (int e = 0; e < 12; ++e) m[e] = best_d >= 0 ? S.best[e] : 0.;
    const double th = p3p_threshold(A.K[4 * b], A.K[4 * b + 1], A.errth);
    int c = 0;
    if (best_d >= 0)
        for (int i = tid; i < n; i += P3P_THREADS) {
            const double d = p3p_point_dist(A, m, o0 + i);
            c += A.mode == 0 ? d <= th : d < th;
        }
    int ninl;
    block_scan(c, sh, &ninl);
    double fro = 0.;   // Sophus::isOrthogonal: |R R^T - I|_F < 1e-10
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double v = m[3 * i] * m[3 * j] + m[3 * i + 1] * m[3 * j + 1] + m[3 * i + 2] * m[3 * j + 2] - (i == j ? 1. : 0.);
            fro += v * v;
        }
    const int status = best_d >= 0 && ninl >= 5 && p3p_sqrt(fro) < 1e-10;
    for (int i = tid; i < n; i += P3P_THREADS) {
        uint8_t o = 0;
        if (status) {
            const double d = p3p_point_dist(A, m, o0 + i);
            o = !(A.mode == 0 ? d <= th : d < th);
        }
        A.outlier[o0 + i] = o;
    }
    if (tid == 0) {
        A.status[b] = status;
        if (status) {
            double q[4];
            ov2se3::rot_to_quat(m, q);
            for (int e = 0; e < 3; ++e) A.Twc[7 * b + e] = m[9 + e];
            for (int e = 0; e < 4; ++e) A.Twc[7 * b + 3 + e] = q[e];
        }
        if (A.info) {
            A.info[4 * b] = S.counted; A.info[4 * b + 1] = S.skipped; A.info[4 * b + 2] = best_d; A.info[4 * b + 3] = ninl;
        }
    }
}

__global__ __launch_bounds__(64) void p3p_dbg_kernel(int n, const double *bv, const double *X, double *R, double *t, int32_t *nsol)
{
    __shared__ p3p_ws W[64];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double f[3][3], P[3][3];
    for (int s = 0; s < 3; ++s)
        for (int k = 0; k < 3; ++k) { f[s][k] = bv[9 * (size_t)i + 3 * s + k]; P[s][k] = X[9 * (size_t)i + 3 * s + k]; }
    double *Ro = R + 36 * (size_t)i, *to = t + 12 * (size_t)i;
    for (int e = 0; e < 36; ++e) Ro[e] = 0.;
    for (int e = 0; e < 12; ++e) to[e] = 0.;
    int k = 0;
    nsol[i] = p3p_kneip(f, P, W[threadIdx.x], [&](const double *r, const double *tt) {
        for (int e = 0; e < 9; ++e) Ro[9 * k + e] = r[e];
        for (int e = 0; e < 3; ++e) to[3 * k + e] = tt[e];
        ++k;
    });
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

extern "C" ov2_status ov2_p3p_ransac_batch_dev(ov2_ctx *c, int B, const int32_t *d_off, const double *d_bvs,
                                               const double *d_wpts, const double *d_K, int nmaxiter, float errth,
                                               int use_lmeds, const uint64_t *d_seed, double *d_Twc, uint8_t *d_outlier,
                                               int32_t *d_status, int32_t *d_info)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || (B && (!d_off || !d_K || !d_seed || !d_Twc || !d_status || !d_bvs || !d_wpts || !d_outlier)))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_p3p_ransac_batch_dev: null argument");
    if (nmaxiter < 0 || nmaxiter > OV2_P3P_MAX_ITER)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_p3p_ransac_batch: nmaxiter %d outside [0, %d]", nmaxiter, OV2_P3P_MAX_ITER);
    if (B > OV2_P3P_MAX_BATCH)   // the frame index is the y dimension of the solve / score grids
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_p3p_ransac_batch: B %d above %d", B, OV2_P3P_MAX_BATCH);
    if (B == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    p3p_args A;
    std::memset(&A, 0, sizeof(A));
    // At most 11 nmaxiter + 1 draws are ever looked at, but the skip budget is rarely touched: the first block holds
    // 2 min(nmaxiter, 256) + 32 draws, which ends the loop unless more than half of them have no model; the blocks behind
    // it (up to 11 min(nmaxiter, 256) + 1 draws each) find their frames done and retire at once.  The workspace is sized
    // for the largest block.
    const int mb = nmaxiter < P3P_MAX_BLOCK_ITER ? nmaxiter : P3P_MAX_BLOCK_ITER;
    const long long total = 11ll * nmaxiter + 1;
    const int d_first = total < 2ll * mb + 32 ? (int)total : 2 * mb + 32;
    A.D = 11 * mb + 1;
    A.L = nmaxiter + 1 < A.D ? nmaxiter + 1 : A.D;
    const size_t o_model = 0, o_valid = up256(sizeof(double) * 12 * (size_t)B * A.D);
    const size_t o_list = o_valid + up256(sizeof(int32_t) * (size_t)B * A.D), o_pen = o_list + up256(sizeof(int32_t) * (size_t)B * A.L);
    const size_t o_st = o_pen + up256(sizeof(double) * (size_t)B * A.L), bytes = o_st + up256(sizeof(p3p_state) * (size_t)B);
    char *ws = nullptr;
    ov2_status s = ov2_scratch(c, bytes, (void **)&ws);
    if (s != OV2_OK) return s;
    A.nmaxiter = nmaxiter; A.mode = use_lmeds ? 0 : 1; A.errth = errth; A.off = d_off; A.bv = d_bvs; A.X = d_wpts; A.K = d_K;
    A.seed = d_seed; A.Twc = d_Twc; A.outlier = d_outlier; A.status = d_status; A.info = d_info;
    A.model = (double *)(ws + o_model); A.valid = (int32_t *)(ws + o_valid); A.list = (int32_t *)(ws + o_list);
    A.pen = (double *)(ws + o_pen); A.st = (p3p_state *)(ws + o_st);
    const int d_max = A.D;
    for (long long d0 = 0; d0 < total; d0 += A.D) {
        A.D = d0 == 0 ? d_first : (total - d0 < d_max ? (int)(total - d0) : d_max);
        A.L = nmaxiter + 1 < A.D ? nmaxiter + 1 : A.D;
        A.d0 = (int)d0; A.first = d0 == 0; A.last = d0 + A.D >= total;
        OV2_LAUNCH(c, K_P3P_SOLVE, p3p_solve_kernel, dim3((A.D + P3P_THREADS - 1) / P3P_THREADS, B), dim3(P3P_THREADS), 0, c->stream, A);
        OV2_LAUNCH(c, K_P3P_SELECT, p3p_select_kernel, dim3(B), dim3(P3P_THREADS), 0, c->stream, A);
        OV2_LAUNCH(c, K_P3P_SCORE, p3p_score_kernel, dim3(A.L, B), dim3(P3P_THREADS), 0, c->stream, A);
        OV2_LAUNCH(c, K_P3P_FINAL, p3p_final_kernel, dim3(B), dim3(P3P_THREADS), 0, c->stream, A);
    }
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

extern "C" ov2_status ov2_p3p_ransac_batch(ov2_ctx *c, int B, const int *n_pts, const double *bvs, const double *wpts,
                                           const double *K, int nmaxiter, float errth, int use_lmeds, const uint64_t *seed,
                                           double *Twc, uint8_t *outlier, int *status, int *info)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || (B && (!n_pts || !K || !seed || !Twc || !status)))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_p3p_ransac_batch: null argument");
    if (nmaxiter < 0 || nmaxiter > OV2_P3P_MAX_ITER)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_p3p_ransac_batch: nmaxiter %d outside [0, %d]", nmaxiter, OV2_P3P_MAX_ITER);
    if (B == 0) return OV2_OK;
    size_t n = 0;
    for (int b = 0; b < B; ++b) {
        if (n_pts[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "negative count");
        n += (size_t)n_pts[b];
    }
    if (n && (!bvs || !wpts || !outlier)) return ov2_set_err(c, OV2_ERR_INVALID, "null point arrays");
    OV2_HIP(c, hipSetDevice(c->device));
    // staging block: [off | K | seed | bvs | wpts | Twc || status | info | outlier]; Twc travels both ways
    const size_t o_off = 0, o_K = up256(sizeof(int) * (B + 1)), o_seed = o_K + up256(sizeof(double) * 4 * B);
    const size_t o_bv = o_seed + up256(sizeof(uint64_t) * B), o_X = o_bv + up256(sizeof(double) * 3 * n);
    const size_t o_T = o_X + up256(sizeof(double) * 3 * n), o_st = o_T + up256(sizeof(double) * 7 * B);
    const size_t o_in = o_st + up256(sizeof(int) * B), o_out = o_in + up256(sizeof(int) * 4 * B), total = o_out + up256(n + 1);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    {
        int *off = (int *)(hp + o_off);
        off[0] = 0;
        for (int b = 0; b < B; ++b) off[b + 1] = off[b] + n_pts[b];
    }
    memcpy(hp + o_K, K, sizeof(double) * 4 * B);
    memcpy(hp + o_seed, seed, sizeof(uint64_t) * B);
    if (n) { memcpy(hp + o_bv, bvs, sizeof(double) * 3 * n); memcpy(hp + o_X, wpts, sizeof(double) * 3 * n); }
    memcpy(hp + o_T, Twc, sizeof(double) * 7 * B);   // untouched where the status is 0
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_st, hipMemcpyHostToDevice, st));
    s = ov2_p3p_ransac_batch_dev(c, B, (const int32_t *)(dp + o_off), (const double *)(dp + o_bv), (const double *)(dp + o_X),
                                 (const double *)(dp + o_K), nmaxiter, errth, use_lmeds, (const uint64_t *)(dp + o_seed),
                                 (double *)(dp + o_T), (uint8_t *)(dp + o_out), (int32_t *)(dp + o_st), (int32_t *)(dp + o_in));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_T, dp + o_T, total - o_T, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(Twc, hp + o_T, sizeof(double) * 7 * B);
    memcpy(status, hp + o_st, sizeof(int) * B);
    if (info) memcpy(info, hp + o_in, sizeof(int) * 4 * B);
    if (n) memcpy(outlier, hp + o_out, n);
    return OV2_OK;
}

extern "C" ov2_status ov2_dbg_p3p(ov2_ctx *c, int n, const double *bv, const double *X, double *R, double *t, int *nsol)
{
    if (!c) return OV2_ERR_INVALID;
    if (n < 0 || (n && (!bv || !X || !R || !t || !nsol))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_dbg_p3p: null argument");
    if (n == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    const size_t o_bv = 0, o_X = up256(sizeof(double) * 9 * n), o_R = o_X + up256(sizeof(double) * 9 * n);
    const size_t o_t = o_R + up256(sizeof(double) * 36 * n), o_ns = o_t + up256(sizeof(double) * 12 * n), total = o_ns + up256(sizeof(int) * n);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    memcpy(hp + o_bv, bv, sizeof(double) * 9 * n);
    memcpy(hp + o_X, X, sizeof(double) * 9 * n);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_R, hipMemcpyHostToDevice, st));
    OV2_LAUNCH(c, K_P3P_DBG, p3p_dbg_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, (const double *)(dp + o_bv),
               (const double *)(dp + o_X), (double *)(dp + o_R), (double *)(dp + o_t), (int32_t *)(dp + o_ns));
    OV2_HIP(c, hipGetLastError());
    OV2_HIP(c, hipMemcpyAsync(hp + o_R, dp + o_R, total - o_R, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(R, hp + o_R, sizeof(double) * 36 * n);
    memcpy(t, hp + o_t, sizeof(double) * 12 * n);
    memcpy(nsol, hp + o_ns, sizeof(int) * n);
    return OV2_OK;
}
