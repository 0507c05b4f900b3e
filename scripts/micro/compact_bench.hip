// Micro-benchmark: what bounds the list compaction in front of the tracking launches (klt_compact_kernel, klt.hip)?
// Back-to-back launches of the kernel alone between two events, per variant and with the two list-length words on one
// 128-byte line (stride 1) or on two (stride 32):
//   one    a keypoint per thread, two returning atomics per 256-keypoint workgroup (the form before DESIGN.md section 7,
//          "Shorter serial kernels per frame")
//   side   eight keypoints per thread side by side (one 8-byte load of their flags), ranks by ballot per slot: the
//          shortest kernel but list entries eight keypoints apart, which the tracking kernels pay for
//   wave   eight keypoints per thread, a wave takes 512 consecutive keypoints (slot k of lane l = keypoint 64 k + l):
//          the kernel in klt.hip, lists ascending inside a workgroup
// The counters run on from launch to launch, so the lists are sized for all launches; the last launch's lists, the zeroed
// work words and the number of descents in list A are checked on the host.
//   build: hipcc -O3 --offload-arch=gfx950 -o build/compact_bench scripts/micro/compact_bench.hip ; run: build/compact_bench [n]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

__global__ __launch_bounds__(256) void one_kernel(int n, const unsigned char *__restrict__ has_prior, unsigned *__restrict__ iters,
                                                  int *__restrict__ list_a, int *__restrict__ list_b, unsigned *__restrict__ cnt, int stride)
{
    __shared__ int wsum[2][4];
    __shared__ int wbase[2];
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool la = false, lb = false;
    if (f < n) {
        const bool hp = has_prior[f] != 0;
        la = hp; lb = !hp;
        iters[hp ? n + f : f] = 0;
    }
    const unsigned long long ma = __ballot(la), mb = __ballot(lb);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int ra = __popcll(ma & below), rb = __popcll(mb & below);
    if (lane == 0) { wsum[0][wv] = __popcll(ma); wsum[1][wv] = __popcll(mb); }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        const int tot = wsum[q][0] + wsum[q][1] + wsum[q][2] + wsum[q][3];
        wbase[q] = tot ? (int)atomicAdd(&cnt[q * stride], (unsigned)tot) : 0;
    }
    __syncthreads();
    int oa = wbase[0], ob = wbase[1];
    for (int k = 0; k < wv; ++k) { oa += wsum[0][k]; ob += wsum[1][k]; }
    if (la) list_a[oa + ra] = f;
    if (lb) list_b[ob + rb] = f;
}

// STEP = 1: slot k of a thread is keypoint 8 t + k; STEP = 64: slot k of lane l of wave w is keypoint 512 w + 64 k + l
template <int STEP>
__global__ __launch_bounds__(256) void eight_kernel(int n, const unsigned char *__restrict__ has_prior, unsigned *__restrict__ iters,
                                                    int *__restrict__ list_a, int *__restrict__ list_b, unsigned *__restrict__ cnt, int stride)
{
    __shared__ int wsum[2][4];
    __shared__ int wbase[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f0 = STEP == 1 ? (blockIdx.x * 256 + threadIdx.x) * 8 : blockIdx.x * 2048 + wv * 512 + lane;
    unsigned char hp[8];
    if (STEP == 1 && f0 + 8 <= n && ((size_t)has_prior & 7) == 0) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long *>(has_prior + f0);
#pragma unroll
        for (int k = 0; k < 8; ++k) hp[k] = (unsigned char)(v >> (8 * k));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) hp[k] = f0 + STEP * k < n ? has_prior[f0 + STEP * k] : 0;
    }
    int pos[8], ta = 0, tb = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool v = f0 + STEP * k < n, p = hp[k] != 0;
        const unsigned long long ba = __ballot(v && p), bb = __ballot(v && !p);
        const int ra = ta + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ba >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ba, 0u));
        const int rb = tb + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bb, 0u));
        ta += __popcll(ba); tb += __popcll(bb);
        pos[k] = p ? ra : rb;
    }
    if (lane == 0) { wsum[0][wv] = ta; wsum[1][wv] = tb; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        const int tot = wsum[q][0] + wsum[q][1] + wsum[q][2] + wsum[q][3];
        wbase[q] = tot ? (int)atomicAdd(&cnt[q * stride], (unsigned)tot) : 0;
    }
    __syncthreads();
    int oa = wbase[0], ob = wbase[1];
    for (int k = 0; k < wv; ++k) { oa += wsum[0][k]; ob += wsum[1][k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int f = f0 + STEP * k;
        if (f < n) {
            const bool p = hp[k] != 0;
            (p ? list_a : list_b)[(p ? oa : ob) + pos[k]] = f;
            iters[p ? n + f : f] = 0;
        }
    }
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 131072, L = 100;
    if (n < 1 || n > (1 << 22)) { printf("n out of range\n"); return 1; }
    std::vector<unsigned char> h(n);
    srand(1);
    for (int i = 0; i < n; ++i) h[i] = (rand() % 10) < 7;
    unsigned char *d_h; unsigned *d_it, *d_cnt; int *d_a, *d_b;
    CK(hipMalloc((void **)&d_h, n));
    CK(hipMalloc((void **)&d_it, 2 * (size_t)n * 4));
    CK(hipMalloc((void **)&d_cnt, 256));
    CK(hipMalloc((void **)&d_a, (size_t)L * n * 4));
    CK(hipMalloc((void **)&d_b, (size_t)L * n * 4));
    CK(hipMemcpy(d_h, h.data(), n, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    const char *names[3] = {"one", "side", "wave"};
    for (int rep = 0; rep < 3; ++rep)
        for (int variant = 0; variant < 3; ++variant)
            for (int stride : {1, 32}) {
                CK(hipMemsetAsync(d_cnt, 0, 256, st));
                CK(hipMemsetAsync(d_it, 0xff, 2 * (size_t)n * 4, st));
                CK(hipEventRecord(e0, st));
                for (int l = 0; l < L; ++l) {
                    if (variant == 0) one_kernel<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(n, d_h, d_it, d_a, d_b, d_cnt, stride);
                    else if (variant == 1) eight_kernel<1><<<dim3((n + 2047) / 2048), dim3(256), 0, st>>>(n, d_h, d_it, d_a, d_b, d_cnt, stride);
                    else eight_kernel<64><<<dim3((n + 2047) / 2048), dim3(256), 0, st>>>(n, d_h, d_it, d_a, d_b, d_cnt, stride);
                }
                CK(hipEventRecord(e1, st));
                CK(hipStreamSynchronize(st));
                CK(hipGetLastError());
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                unsigned c[64];
                CK(hipMemcpy(c, d_cnt, 256, hipMemcpyDeviceToHost));
                const size_t na = c[0] / L, nb = c[stride] / L;
                bool ok = na + nb == (size_t)n;
                std::vector<int> la(ok ? na : 0), lb(ok ? nb : 0), seen(n, 0);
                std::vector<unsigned> it(2 * (size_t)n);
                if (ok && na) CK(hipMemcpy(la.data(), d_a + (size_t)(L - 1) * na, na * 4, hipMemcpyDeviceToHost));
                if (ok && nb) CK(hipMemcpy(lb.data(), d_b + (size_t)(L - 1) * nb, nb * 4, hipMemcpyDeviceToHost));
                CK(hipMemcpy(it.data(), d_it, it.size() * 4, hipMemcpyDeviceToHost));
                for (int v : la) { if (v < 0 || v >= n || !h[v]) ok = false; else seen[v]++; }
                for (int v : lb) { if (v < 0 || v >= n || h[v]) ok = false; else seen[v]++; }
                for (int i = 0; i < n; ++i)
                    if (seen[i] != 1 || it[h[i] ? n + i : i] != 0u || it[h[i] ? i : n + i] != 0xffffffffu) ok = false;
                int descents = 0;
                for (size_t i = 1; i < la.size(); ++i) descents += la[i] < la[i - 1];
                printf("n %d run %d %-4s counters %3d B apart: %.2f us per launch, lists %zu + %zu %s, %d descents in list A\n", n, rep,
                       names[variant], 4 * stride, 1000.f * ms / L, na, nb, ok ? "ok" : "WRONG", descents);
            }
    return 0;
}
