// knn.hip -- ov2_knn2_hamming_batch: the two nearest train descriptors of every query descriptor by Hamming distance, B
// independent (query set, train set) pairs per launch.  Replaces cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train,
// vmatches, 2) of LoopCloser::knnMatching (src/loop_closer.cpp:426-428).
//
// One launch, no atomics.  A workgroup of 256 threads owns 256 / LANES consecutive rows of the concatenated query array;
// LANES (1 | 4 | 16 | 64) lanes share one query, whose 32 bytes each of them holds in 8 registers, and split the train
// rows of a tile between them (lane s takes rows s, s + LANES, ...).  The train rows of the pair travel through LDS in
// tiles of KNN_TILE rows; every row is read with two ds_read_b128.  With LANES == 1 all lanes of a wave read one address
// (a broadcast); with more lanes per query, the lanes of a ds_read_b128 group read up to 16 different rows, and the two
// 16-byte halves of rows 8-15 (mod 16) are stored swapped so that those reads fall on 16 different 4-bank slots.
// A lane keeps the two smallest keys (dist << 16) | idx it has seen; keys of one query are distinct, so the two smallest
// of a union are the same whatever the order of the merge: the lanes of a query merge through ov2wave::row_min2_i32 /
// wave_min2_i32.  A workgroup whose query rows straddle pairs walks those pairs one after the other.
#include "ov2_internal.h"
#include "ov2_wave.h"

namespace {

enum { KNN_THREADS = 256, KNN_TILE = OV2_KNN_TILE, K_KNN2 = OV2_K_MAP + 14 };
#define KNN_NONE 0x7fffffff   // above every key: dist <= 256 and idx < 65536

struct knn_args {
    int B, total_q;
    const int32_t *q_off, *t_off;   // B + 1 prefix offsets (rows)
    const uint4 *query, *train;     // 2 x uint4 per row
    int32_t *idx, *dist;            // 2 per query row
};

__device__ __forceinline__ int popc4(const uint4 a, const uint4 b)
{
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

template <int LANES>
__global__ __launch_bounds__(KNN_THREADS) void knn2_kernel(const knn_args A)
{
    __shared__ uint4 tile[KNN_TILE * 2];
    constexpr int QPB = KNN_THREADS / LANES;
    const int t = threadIdx.x, sub = t & (LANES - 1);
    const int nq_all = min(A.total_q, A.q_off[A.B]);
    const int q_lo = blockIdx.x * QPB, q_hi = min(q_lo + QPB, nq_all);
    if (q_lo >= q_hi) return;   // whole workgroup
    const int q = q_lo + t / LANES;
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (q < q_hi) { qa = A.query[2 * (size_t)q]; qb = A.query[2 * (size_t)q + 1]; }
    // the last pair that starts at or before q_lo (uniform); q_off[0] = 0
    int p = 0;
    for (int hi = A.B - 1; p < hi;) {
        const int mid = (p + hi + 1) >> 1;
        if (A.q_off[mid] <= q_lo) p = mid; else hi = mid - 1;
    }
    for (; p < A.B && A.q_off[p] < q_hi; ++p) {
        const int q0 = A.q_off[p], q1 = A.q_off[p + 1];
        if (q1 <= q_lo || q1 <= q0) continue;   // a pair without query rows here
        const int t0 = A.t_off[p];
        const int nt = min(A.t_off[p + 1] - t0, (int)OV2_KNN_MAX_TRAIN);
        const bool mine = q >= q0 && q < q1 && q < q_hi;
        int k0 = KNN_NONE, k1 = KNN_NONE;
        for (int base = 0; base < nt; base += KNN_TILE) {
            const int rows = min((int)KNN_TILE, nt - base);
            __syncthreads();   // the tile before this one has been read
            for (int i = t; i < 2 * rows; i += KNN_THREADS) {
                const int r = i >> 1;
                tile[i ^ ((r >> 3) & 1)] = A.train[2 * (size_t)(t0 + base) + i];
            }
            __syncthreads();
            if (mine) {
#pragma unroll 4
                for (int j = sub; j < rows; j += LANES) {
                    const int sw = (j >> 3) & 1;
                    const uint4 ta = tile[2 * j + sw], tb = tile[2 * j + (sw ^ 1)];
                    const int key = ((popc4(qa, ta) + popc4(qb, tb)) << 16) | (base + j);
                    k1 = min(k1, max(k0, key));
                    k0 = min(k0, key);
                }
            }
        }
        if constexpr (LANES == 64) ov2wave::wave_min2_i32(k0, k1);
        else if constexpr (LANES > 1) ov2wave::row_min2_i32<LANES>(k0, k1);
        if (mine && sub == 0) {
            A.idx[2 * (size_t)q] = k0 == KNN_NONE ? -1 : (k0 & 0xffff);
            A.dist[2 * (size_t)q] = k0 == KNN_NONE ? -1 : (k0 >> 16);
            A.idx[2 * (size_t)q + 1] = k1 == KNN_NONE ? -1 : (k1 & 0xffff);
            A.dist[2 * (size_t)q + 1] = k1 == KNN_NONE ? -1 : (k1 >> 16);
        }
    }
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// Lanes per query when ov2_knn_set_lanes is 0: the fewest lanes that still give every compute unit the context runs on
// (its CU share, else the device: ov2_ctx::knn_cus) a workgroup.  Measured on an MI355X (scripts/knn_time.py, profiles/README.md).
int knn_lanes_for(const ov2_ctx *c, int total_q)
{
    if (c->knn_lanes) return c->knn_lanes;
    for (int lanes = 1; lanes < 64; lanes *= 4)
        if ((long long)total_q * lanes >= (long long)KNN_THREADS * c->knn_cus) return lanes;
    return 64;
}

ov2_status knn_cus(ov2_ctx *c)
{
    if (!c->knn_cus) {
        int cus = 0;
        OV2_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->knn_cus = cus > 0 ? cus : 1;
    }
    return OV2_OK;
}

}  // namespace

extern "C" int ov2_knn_lanes_for(ov2_ctx *c, int total_query)
{
    if (!c || total_query < 0 || knn_cus(c) != OV2_OK) return -1;
    return knn_lanes_for(c, total_query);
}

extern "C" ov2_status ov2_knn_set_lanes(ov2_ctx *c, int lanes)
{
    if (!c) return OV2_ERR_INVALID;
    if (lanes != 0 && lanes != 1 && lanes != 4 && lanes != 16 && lanes != 64)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn_set_lanes: %d is none of 0, 1, 4, 16, 64", lanes);
    c->knn_lanes = lanes;
    return OV2_OK;
}

extern "C" ov2_status ov2_knn2_hamming_batch_dev(ov2_ctx *c, int B, int total_query, const int32_t *d_q_off,
                                                 const int32_t *d_t_off, const uint8_t *d_query, const uint8_t *d_train,
                                                 int32_t *d_idx, int32_t *d_dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || total_query < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch_dev: negative count");
    if (B > OV2_KNN_MAX_BATCH) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: B %d above %d", B, OV2_KNN_MAX_BATCH);
    if (total_query > OV2_KNN_MAX_ROWS)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: %d query rows above %d", total_query, OV2_KNN_MAX_ROWS);
    if (B && (!d_q_off || !d_t_off)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch_dev: null offsets");
    if (total_query && (!B || !d_query || !d_idx || !d_dist))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch_dev: null argument");
    if (((uintptr_t)d_query | (uintptr_t)d_train) & 15)   // rows are read 16 bytes at a time
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch_dev: descriptor arrays must be 16-byte aligned");
    if (B == 0 || total_query == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    const ov2_status cs = knn_cus(c);
    if (cs != OV2_OK) return cs;
    knn_args A;
    A.B = B; A.total_q = total_query; A.q_off = d_q_off; A.t_off = d_t_off;
    A.query = (const uint4 *)d_query; A.train = (const uint4 *)d_train; A.idx = d_idx; A.dist = d_dist;
    const int lanes = knn_lanes_for(c, total_query);
    const dim3 grid((unsigned)(((long long)total_query * lanes + KNN_THREADS - 1) / KNN_THREADS)), block(KNN_THREADS);
    switch (lanes) {
    case 1: OV2_LAUNCH(c, K_KNN2, knn2_kernel<1>, grid, block, 0, c->stream, A); break;
    case 4: OV2_LAUNCH(c, K_KNN2, knn2_kernel<4>, grid, block, 0, c->stream, A); break;
    case 16: OV2_LAUNCH(c, K_KNN2, knn2_kernel<16>, grid, block, 0, c->stream, A); break;
    default: OV2_LAUNCH(c, K_KNN2, knn2_kernel<64>, grid, block, 0, c->stream, A); break;
    }
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

extern "C" ov2_status ov2_knn2_hamming_batch(ov2_ctx *c, int B, const int *n_query, const int *n_train, const uint8_t *query,
                                             const uint8_t *train, int32_t *idx, int32_t *dist)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || (B && (!n_query || !n_train))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: null argument");
    if (B > OV2_KNN_MAX_BATCH) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: B %d above %d", B, OV2_KNN_MAX_BATCH);
    if (B == 0) return OV2_OK;
    size_t nq = 0, nt = 0;
    for (int b = 0; b < B; ++b) {
        if (n_query[b] < 0 || n_train[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: negative count");
        if (n_train[b] > OV2_KNN_MAX_TRAIN)
            return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: pair %d has %d train rows, above %d", b, n_train[b],
                               OV2_KNN_MAX_TRAIN);
        nq += (size_t)n_query[b];
        nt += (size_t)n_train[b];
        if (nq > OV2_KNN_MAX_ROWS || nt > OV2_KNN_MAX_ROWS)
            return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: more than %d rows", OV2_KNN_MAX_ROWS);
    }
    if ((nq && (!query || !idx || !dist)) || (nt && !train)) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_knn2_hamming_batch: null array");
    if (nq == 0) return OV2_OK;
    // staging block: [q_off | t_off | query | train || idx | dist]
    const size_t o_qo = 0, o_to = up256(sizeof(int32_t) * (B + 1)), o_q = o_to + up256(sizeof(int32_t) * (B + 1));
    const size_t o_t = o_q + up256(32 * nq), o_idx = o_t + up256(32 * nt), o_dist = o_idx + up256(8 * nq), total = o_dist + up256(8 * nq);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    int32_t *qo = (int32_t *)(hp + o_qo), *to = (int32_t *)(hp + o_to);
    qo[0] = to[0] = 0;
    for (int b = 0; b < B; ++b) { qo[b + 1] = qo[b] + n_query[b]; to[b + 1] = to[b] + n_train[b]; }
    memcpy(hp + o_q, query, 32 * nq);
    if (nt) memcpy(hp + o_t, train, 32 * nt);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_idx, hipMemcpyHostToDevice, st));
    s = ov2_knn2_hamming_batch_dev(c, B, (int)nq, (const int32_t *)(dp + o_qo), (const int32_t *)(dp + o_to), (const uint8_t *)(dp + o_q),
                                   (const uint8_t *)(dp + o_t), (int32_t *)(dp + o_idx), (int32_t *)(dp + o_dist));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_idx, dp + o_idx, total - o_idx, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(idx, hp + o_idx, 8 * nq);
    memcpy(dist, hp + o_dist, 8 * nq);
    return OV2_OK;
}
