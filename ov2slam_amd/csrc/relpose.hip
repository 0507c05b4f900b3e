// relpose.hip -- refinement of a two-view relative pose [R | t], |t| = 1, on the inliers of the 5-point RANSAC, on gfx950:
// the whole Levenberg-Marquardt loop on device, B frames per launch.
//
// Stands where the reference calls compute5ptEssentialMatrix(..., do_optimize = true, ...) (reference
// src/visual_front_end.cpp:537-544 and :855-984 -> src/multi_view_geometry.cpp:672-681, OpenGV's
// optimizeModelCoefficients).  DEVIATION: OpenGV's cost is not restated (its source is not in the reference tree); the cost
// here is the Sampson distance on the sphere, in pixels (include/ov2slam_hip.h, ov2_relpose_refine_batch).
//
// A sibling of pnp_kernel (pnp.hip): one workgroup (256 threads) per frame, the pose and the 5x5 system in registers of
// every thread (wave-uniform), pairs strided over the threads, the 21 sums (cost, J'r, upper J'J) reduced in the fixed
// order of pnp.hip's block_sum (DPP row sums -> readlane -> LDS across the 4 waves), the scalar LM logic executed
// redundantly by all threads: no atomics, no host round trip, no divergence.  The jacobian is never stored.  f64 throughout.
#include "ov2_internal.h"
#include "ov2_se3.h"
#include "ov2_wave.h"

using namespace ov2se3;
using namespace ov2wave;

namespace {

enum { RP_THREADS = 256, RP_SUMS = 21, RP_MIN_PAIRS = 6, K_RELPOSE = OV2_K_BA_FIRST + 12 };

struct rp_params {
    int max_iters, max_invalid;
    double ftol, initial_radius, max_radius, min_radius, min_diag, max_diag, min_rel, ptol;
};

struct rp_args {
    const int32_t *off;
    const double *bv_kf, *bv_cur;
    const uint8_t *skip;
    const double *K;
    const int32_t *in_status;
    double *R, *t;
    int32_t *status, *info;
    double *cost;
    rp_params P;
};

// acc[K] of every thread -> block totals in every thread, in pnp.hip's order
template <int K>
__device__ __forceinline__ void rp_block_sum(double *acc, double (*sh)[RP_SUMS])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum_f64(acc[k]);
        if ((tid & 63) == 0) sh[tid >> 6][k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
    __syncthreads();
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// b1 = normalise(e_k x t), k = index of the smallest |t_k| (lowest index on a tie); b2 = t x b1
__device__ __forceinline__ void rp_basis(const double *t, double *b1, double *b2)
{
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    int k = 0;
    double am = a0;
    if (a1 < am) { k = 1; am = a1; }
    if (a2 < am) k = 2;
    // e_k x t
    if (k == 0) { b1[0] = 0.0; b1[1] = -t[2]; b1[2] = t[1]; }
    else if (k == 1) { b1[0] = t[2]; b1[1] = 0.0; b1[2] = -t[0]; }
    else { b1[0] = -t[1]; b1[1] = t[0]; b1[2] = 0.0; }
    const double n = sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
    b1[0] /= n; b1[1] /= n; b1[2] /= n;
    cross3(t, b1, b2);
}

// x = [t, qx qy qz qw] -> x (+) (w, a, b)
__device__ __forceinline__ void rp_plus(const double *x, const double *d, double *out)
{
    double b1[3], b2[3];
    rp_basis(x, b1, b2);
    quat_plus_left(x + 3, d, out + 3);
    double tn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) tn[k] = x[k] + d[3] * b1[k] + d[4] * b2[k];
    const double n = sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
    out[0] = tn[0] / n; out[1] = tn[1] / n; out[2] = tn[2] / n;
}

struct rp_frame {
    int i0, i1;
    const double *f1, *f2;
    const uint8_t *skip;
    double focal;
};

// acc = {cost, g[5], H upper triangle [15]} at x (JAC) or {cost} only
template <bool JAC>
__device__ __forceinline__ void rp_accumulate(const rp_frame &F, const double *x, double *acc)
{
    double R[9], b1[3], b2[3];
    quat_to_R(x + 3, R);
    const double *t = x;
    if (JAC) rp_basis(t, b1, b2);
#pragma unroll
    for (int k = 0; k < (JAC ? RP_SUMS : 1); ++k) acc[k] = 0.0;
    for (int i = F.i0 + (int)threadIdx.x; i < F.i1; i += RP_THREADS) {
        if (F.skip && F.skip[i]) continue;
        const double *p1 = F.f1 + 3 * (size_t)i, *p2 = F.f2 + 3 * (size_t)i;
        const double f1[3] = {p1[0], p1[1], p1[2]}, f2[3] = {p2[0], p2[1], p2[2]};
        const double g[3] = {R[0] * f2[0] + R[1] * f2[1] + R[2] * f2[2], R[3] * f2[0] + R[4] * f2[1] + R[5] * f2[2],
                             R[6] * f2[0] + R[7] * f2[1] + R[8] * f2[2]};
        double m[3], w[3];
        cross3(t, g, m);
        cross3(f1, t, w);
        const double u[3] = {R[0] * w[0] + R[3] * w[1] + R[6] * w[2], R[1] * w[0] + R[4] * w[1] + R[7] * w[2],
                             R[2] * w[0] + R[5] * w[1] + R[8] * w[2]};
        const double c = dot3(f1, m), e = dot3(u, f2);
        const double D = dot3(m, m) - c * c + dot3(u, u) - e * e;
        if (!(D > 0.0 && isfinite(D))) continue;   // contributes nothing to this evaluation
        const double s = 1.0 / sqrt(D);
        const double r = F.focal * c * s;
        acc[0] += 0.5 * (r * r);
        if (!JAC) continue;
        double Aw[3], At[3], mt[3], gmt[3], gm[3], wf[3];
        cross3(g, w, Aw);        // dc / dw
        cross3(m, t, mt);
        cross3(g, mt, gmt);
        cross3(g, f1, At);       // dc / dt
        cross3(g, m, gm);
        cross3(w, f1, wf);
        const double ce = c + e, h = 0.5 * c * s * s * s;
        double Jt[3], J[5];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double Dw = 2.0 * (gmt[k] - ce * Aw[k]);
            const double Dt = 2.0 * (gm[k] + wf[k] - ce * At[k]);
            J[k] = F.focal * (s * Aw[k] - h * Dw);
            Jt[k] = F.focal * (s * At[k] - h * Dt);
        }
        J[3] = dot3(Jt, b1);
        J[4] = dot3(Jt, b2);
        int q = 6;
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            acc[1 + a] += J[a] * r;
#pragma unroll
            for (int b = a; b < 5; ++b) acc[q++] += J[a] * J[b];
        }
    }
}

__device__ __forceinline__ bool chol5(const double *A, const double *b, double *x)
{
    double L[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) L[i] = A[i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double d = L[j * 5 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * 5 + k] * L[j * 5 + k];
        if (!(d > 0.0)) ok = false;
        d = sqrt(d > 0.0 ? d : 1.0);
        L[j * 5 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 5; ++i) {
            double s = L[i * 5 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i * 5 + k] * L[j * 5 + k];
            L[i * 5 + j] = s / d;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i * 5 + k] * x[k];
        x[i] = s / L[i * 5 + i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < 5; ++k) s -= L[k * 5 + i] * x[k];
        x[i] = s / L[i * 5 + i];
    }
    return ok;
}

__global__ __launch_bounds__(RP_THREADS) void relpose_kernel(int B, rp_args A)
{
    __shared__ double sh[4][RP_SUMS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;
    const rp_params &P = A.P;
    rp_frame F;
    F.i0 = A.off[b]; F.i1 = A.off[b + 1];
    F.f1 = A.bv_kf; F.f2 = A.bv_cur; F.skip = A.skip;
    F.focal = (A.K[4 * b] + A.K[4 * b + 1]) / 2.0;

    int n_iter = 0, term = OV2_BA_TERM_SKIPPED, accepted = 0;
    double cost0 = 0.0, x_cost = 0.0, x[7];
    bool run = !(A.in_status && A.in_status[b] < 1);
    if (run) {   // admitted pairs and non-finite input, one block-wide count each
        double cnt[2] = {0.0, 0.0};
        for (int i = F.i0 + tid; i < F.i1; i += RP_THREADS) {
            if (F.skip && F.skip[i]) continue;
            cnt[0] += 1.0;
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fin = fin && isfinite(F.f1[3 * (size_t)i + k]) && isfinite(F.f2[3 * (size_t)i + k]);
            if (!fin) cnt[1] += 1.0;
        }
        rp_block_sum<2>(cnt, sh);
        double R0[9], t0[3];
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) { R0[k] = A.R[9 * b + k]; fin = fin && isfinite(R0[k]); }
#pragma unroll
        for (int k = 0; k < 3; ++k) { t0[k] = A.t[3 * b + k]; fin = fin && isfinite(t0[k]); }
        const double tn = sqrt(t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2]);
        run = cnt[0] >= (double)RP_MIN_PAIRS && cnt[1] == 0.0 && fin && isfinite(tn) && tn > 0.0 && isfinite(F.focal);
        if (run) {
            double q[4];
            rot_to_quat(R0, q);
            const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            x[0] = t0[0] / tn; x[1] = t0[1] / tn; x[2] = t0[2] / tn;
            x[3] = q[0] / nq; x[4] = q[1] / nq; x[5] = q[2] / nq; x[6] = q[3] / nq;
        }
    }
    if (run) {   // TrustRegionMinimizer, the rules of pnp_minimize
        double acc[RP_SUMS], H[25], g[5], scale[5], diag[5];
        auto unpack = [&]() {
            int t = 6;
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                g[p] = acc[1 + p];
#pragma unroll
                for (int q = p; q < 5; ++q) { H[p * 5 + q] = acc[t]; H[q * 5 + p] = acc[t]; ++t; }
            }
        };
        rp_accumulate<true>(F, x, acc);
        rp_block_sum<RP_SUMS>(acc, sh);
        x_cost = cost0 = acc[0];
        unpack();
        term = OV2_BA_TERM_MAX_ITER;
        if (!isfinite(x_cost)) { term = OV2_BA_TERM_SKIPPED; cost0 = x_cost = 0.0; }
        else {
#pragma unroll
            for (int c = 0; c < 5; ++c) scale[c] = 1.0 / (1.0 + sqrt(H[c * 5 + c]));
            double x_norm = -1.0, radius = P.initial_radius, dec = 2.0;
            int reuse = 0, invalid = 0, iteration = 0;
            for (;;) {
                if (iteration >= P.max_iters) { term = OV2_BA_TERM_MAX_ITER; break; }
                if (radius <= P.min_radius) { term = OV2_BA_TERM_MIN_RADIUS; break; }
                ++iteration;
                n_iter = iteration;
                double Hs[25], gs[5], M[25], y[5], step[5];
#pragma unroll
                for (int p = 0; p < 5; ++p) {
                    gs[p] = g[p] * scale[p];
#pragma unroll
                    for (int q = 0; q < 5; ++q) Hs[p * 5 + q] = H[p * 5 + q] * scale[p] * scale[q];
                }
                if (!reuse) {
#pragma unroll
                    for (int c = 0; c < 5; ++c) diag[c] = fmin(fmax(Hs[c * 5 + c], P.min_diag), P.max_diag);
                }
                reuse = 1;
#pragma unroll
                for (int k = 0; k < 25; ++k) M[k] = Hs[k];
#pragma unroll
                for (int c = 0; c < 5; ++c) M[c * 5 + c] += diag[c] / radius;
                bool ok = chol5(M, gs, y);
                double model_change = 0.0;
#pragma unroll
                for (int p = 0; p < 5; ++p) { step[p] = -y[p]; if (!isfinite(step[p])) ok = false; }
                if (ok) {
                    double sg = 0, shs = 0;
#pragma unroll
                    for (int p = 0; p < 5; ++p) {
                        sg += step[p] * gs[p];
#pragma unroll
                        for (int q = 0; q < 5; ++q) shs += step[p] * Hs[p * 5 + q] * step[q];
                    }
                    model_change = -(sg + 0.5 * shs);
                }
                if (!ok || !(model_change > 0.0)) {
                    if (++invalid >= P.max_invalid) { term = OV2_BA_TERM_FAILURE; break; }
                    radius /= dec; dec *= 2.0;
                    continue;
                }
                invalid = 0;
                double delta[5], cand[7], cacc[1];
#pragma unroll
                for (int c = 0; c < 5; ++c) delta[c] = step[c] * scale[c];
                rp_plus(x, delta, cand);
                rp_accumulate<false>(F, cand, cacc);
                rp_block_sum<1>(cacc, sh);
                const double cand_cost = cacc[0];
                double sn = 0;
#pragma unroll
                for (int c = 0; c < 7; ++c) sn += (x[c] - cand[c]) * (x[c] - cand[c]);
                if (sqrt(sn) <= P.ptol * (x_norm + P.ptol)) { term = OV2_BA_TERM_PTOL; break; }
                const double cost_change = x_cost - cand_cost;
                if (fabs(cost_change) <= P.ftol * x_cost) { term = OV2_BA_TERM_FTOL; break; }
                const double rel = cost_change / model_change;
                if (rel > P.min_rel) {
                    x_norm = 0;
#pragma unroll
                    for (int c = 0; c < 7; ++c) { x[c] = cand[c]; x_norm += x[c] * x[c]; }
                    x_norm = sqrt(x_norm);
                    rp_accumulate<true>(F, x, acc);
                    rp_block_sum<RP_SUMS>(acc, sh);
                    x_cost = acc[0];
                    unpack();
                    radius = fmin(P.max_radius, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3.0)));
                    dec = 2.0; reuse = 0;
                    ++accepted;
                } else {
                    radius /= dec; dec *= 2.0;
                }
            }
        }
    }
    if (accepted > 0) {   // R, t stay bit-untouched otherwise
        double R[9];
        quat_to_R(x + 3, R);
        if (tid < 9) A.R[9 * b + tid] = R[tid];
        if (tid < 3) A.t[3 * b + tid] = x[tid];
    }
    if (tid == 0) {
        A.status[b] = accepted > 0 ? 1 : 0;
        if (A.info) { A.info[2 * b] = n_iter; A.info[2 * b + 1] = term; }
        if (A.cost) { A.cost[2 * b] = cost0; A.cost[2 * b + 1] = x_cost; }
    }
}

}  // namespace

// device-resident, asynchronous form: every array already in HBM, nothing synchronised
extern "C" ov2_status ov2_relpose_refine_batch_dev(ov2_ctx *c, int B, const int32_t *d_off, const double *d_bv_kf,
                                                   const double *d_bv_cur, const uint8_t *d_skip, const double *d_K,
                                                   int max_iters, const int32_t *d_in_status, double *d_R_kfc,
                                                   double *d_t_kfc, int32_t *d_status, int32_t *d_info, double *d_cost)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || max_iters < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: negative argument");
    if (B && (!d_off || !d_bv_kf || !d_bv_cur || !d_K || !d_R_kfc || !d_t_kfc || !d_status))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch_dev: null argument");
    if (B == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_ba_options o;
    ov2_ba_default_options(&o, 5.9915f);   // the trust-region constants of the motion-only BA; no loss here
    rp_args A;
    A.off = d_off; A.bv_kf = d_bv_kf; A.bv_cur = d_bv_cur; A.skip = d_skip; A.K = d_K; A.in_status = d_in_status;
    A.R = d_R_kfc; A.t = d_t_kfc; A.status = d_status; A.info = d_info; A.cost = d_cost;
    // function_tolerance: Ceres' default, not the 1e-3 the reference sets for its BA problems (include/ov2slam_hip.h)
    A.P.max_iters = max_iters; A.P.max_invalid = o.max_consecutive_invalid_steps; A.P.ftol = OV2_RELPOSE_FUNCTION_TOLERANCE;
    A.P.initial_radius = o.initial_radius; A.P.max_radius = o.max_radius; A.P.min_radius = o.min_radius;
    A.P.min_diag = o.min_lm_diagonal; A.P.max_diag = o.max_lm_diagonal; A.P.min_rel = o.min_relative_decrease;
    A.P.ptol = o.parameter_tolerance;
    OV2_LAUNCH(c, K_RELPOSE, relpose_kernel, dim3(B), dim3(RP_THREADS), 0, c->stream, B, A);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

// host-pointer form: arguments staged through pinned memory (one copy in, one copy out, one synchronisation)
extern "C" ov2_status ov2_relpose_refine_batch(ov2_ctx *c, int B, const int *n_pairs, const double *bv_kf,
                                               const double *bv_cur, const uint8_t *skip, const double *K, int max_iters,
                                               double *R_kfc, double *t_kfc, int *status, int *info, double *cost)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || max_iters < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: negative argument");
    if (B && (!n_pairs || !K || !R_kfc || !t_kfc || !status))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: null argument");
    if (B == 0) return OV2_OK;
    size_t n = 0;
    for (int b = 0; b < B; ++b) {
        if (n_pairs[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: negative pair count");
        n += (size_t)n_pairs[b];
    }
    if (n > (size_t)INT32_MAX) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: too many pairs");
    if (n && (!bv_kf || !bv_cur)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_relpose_refine_batch: null pair arrays");
    OV2_HIP(c, hipSetDevice(c->device));
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // staging block: [off | K | bv_kf | bv_cur | skip || R | t | status | info | cost]
    const size_t o_off = 0, o_K = up(sizeof(int) * (B + 1)), o_b1 = o_K + up(sizeof(double) * 4 * B);
    const size_t o_b2 = o_b1 + up(sizeof(double) * 3 * n), o_sk = o_b2 + up(sizeof(double) * 3 * n), o_R = o_sk + up(n);
    const size_t o_t = o_R + up(sizeof(double) * 9 * B), o_st = o_t + up(sizeof(double) * 3 * B);
    const size_t o_in = o_st + up(sizeof(int) * B), o_co = o_in + up(sizeof(int) * 2 * B);
    const size_t total = o_co + up(sizeof(double) * 2 * B);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    {
        int *off = (int *)(hp + o_off);
        off[0] = 0;
        for (int b = 0; b < B; ++b) off[b + 1] = off[b] + n_pairs[b];
    }
    memcpy(hp + o_K, K, sizeof(double) * 4 * B);
    if (n) {
        memcpy(hp + o_b1, bv_kf, sizeof(double) * 3 * n);
        memcpy(hp + o_b2, bv_cur, sizeof(double) * 3 * n);
        if (skip) memcpy(hp + o_sk, skip, n);
    }
    memcpy(hp + o_R, R_kfc, sizeof(double) * 9 * B);   // come back as they went where the status is 0
    memcpy(hp + o_t, t_kfc, sizeof(double) * 3 * B);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_st, hipMemcpyHostToDevice, st));
    s = ov2_relpose_refine_batch_dev(c, B, (const int32_t *)(dp + o_off), (const double *)(dp + o_b1),
                                     (const double *)(dp + o_b2), (skip && n) ? (const uint8_t *)(dp + o_sk) : nullptr,
                                     (const double *)(dp + o_K), max_iters, nullptr, (double *)(dp + o_R),
                                     (double *)(dp + o_t), (int32_t *)(dp + o_st), (int32_t *)(dp + o_in),
                                     (double *)(dp + o_co));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_R, dp + o_R, total - o_R, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(R_kfc, hp + o_R, sizeof(double) * 9 * B);
    memcpy(t_kfc, hp + o_t, sizeof(double) * 3 * B);
    memcpy(status, hp + o_st, sizeof(int) * B);
    if (info) memcpy(info, hp + o_in, sizeof(int) * 2 * B);
    if (cost) memcpy(cost, hp + o_co, sizeof(double) * 2 * B);
    return OV2_OK;
}
