// Probe: what does a CU mask on a HIP stream do on this device?  (ov2_ctx_create_cu, ov2_cu_mask_build)
// On streams created with hipExtStreamCreateWithCUMask it launches
//   where_kernel   4096 one-wave workgroups that each note the XCD (HW_REG_XCC_ID) and the shader engine / array / CU
//                  (HW_REG_HW_ID) they ran on, after a short VALU loop so that one compute unit cannot drain the grid alone
//   valu_kernel    a fixed VALU loop (2048 workgroups of 256 threads), timed with events
// and prints
//   1. for single-bit masks (bits 0 .. 15 and the last bit): the compute units seen per XCD and the one of XCD k % 8 --
//      the bit-to-CU mapping;
//   2. for the masks of ov2_cu_mask_build, both layouts, n = 8, 32, 64, 128: the mask HIP reports back, the number of
//      distinct compute units seen, the compute units seen per XCD, and the time of the VALU loop, which must fall as
//      1 / (compute units seen) if the mask confines the kernel;
//   3. the same two kernels on a stream without a mask.
// One process, a few seconds.  Exit status 0 when every mask did what the rule in main() says (an XCD runs on as many
// compute units as the mask gives it bits, on all of its own when it has none), 1 otherwise.
//   build: hipcc -O3 --offload-arch=gfx950 -Iinclude -o build/cu_mask_probe scripts/micro/cu_mask_probe.hip \
//          -Lov2slam_amd/lib -lov2hip -Wl,-rpath,'$ORIGIN/../ov2slam_amd/lib'
//   run:   timeout -k 10 120 build/cu_mask_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "ov2slam_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

constexpr int WHERE_BLOCKS = 4096;
constexpr int VALU_BLOCKS = 2048, VALU_ITERS = 16000;
constexpr int MAX_WORDS = 32;

__global__ __launch_bounds__(64) void where_kernel(unsigned *__restrict__ out, float seed)
{
    float a = seed + (float)threadIdx.x;
    for (int i = 0; i < 4000; ++i) a = a * 1.0001f + 0.5f;
    unsigned xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = xcc;
        out[2 * blockIdx.x + 1] = hw + (a == 12345.678f ? 1u : 0u);   // keeps the loop alive
    }
}

__global__ __launch_bounds__(256) void valu_kernel(float *__restrict__ out, float seed)
{
    float a = seed + (float)threadIdx.x, b = a + 1.f, c = a + 2.f, d = a + 3.f;
    for (int i = 0; i < VALU_ITERS; ++i) {
        a = a * 1.0001f + 0.5f;
        b = b * 1.0002f + 0.25f;
        c = c * 0.9999f + 0.125f;
        d = d * 0.9998f + 0.0625f;
    }
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = a + b + c + d;
}

struct cu_id {
    int xcd, se, sh, cu;
    bool operator<(const cu_id &o) const { return std::tie(xcd, se, sh, cu) < std::tie(o.xcd, o.se, o.sh, o.cu); }
};

static unsigned *d_where;
static float *d_valu;
static hipEvent_t ev0, ev1;

// runs both kernels on `st`; the compute units seen and the time of the VALU loop
static std::set<cu_id> run_on(hipStream_t st, float *ms)
{
    std::vector<unsigned> h(2 * WHERE_BLOCKS);
    hipLaunchKernelGGL(where_kernel, dim3(WHERE_BLOCKS), dim3(64), 0, st, d_where, 1.0f);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(h.data(), d_where, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(valu_kernel, dim3(VALU_BLOCKS), dim3(256), 0, st, d_valu, 1.0f);   // warm-up: code object, clocks
    CK(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(valu_kernel, dim3(VALU_BLOCKS), dim3(256), 0, st, d_valu, 2.0f);
    CK(hipEventRecord(ev1, st));
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(ms, ev0, ev1));
    std::set<cu_id> seen;
    for (int b = 0; b < WHERE_BLOCKS; ++b) {
        const unsigned xcc = h[2 * b], hw = h[2 * b + 1];
        seen.insert(cu_id{(int)(xcc & 0xf), (int)((hw >> 13) & 0x7), (int)((hw >> 12) & 0x1), (int)((hw >> 8) & 0xf)});
    }
    return seen;
}

static void per_xcd(const std::set<cu_id> &seen, int cnt[OV2_CU_MASK_XCDS])
{
    for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) cnt[x] = 0;
    for (const cu_id &c : seen)
        if (c.xcd < OV2_CU_MASK_XCDS) ++cnt[c.xcd];
}

int main()
{
    int dev = 0, total = 0;
    CK(hipSetDevice(dev));
    CK(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, dev));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, dev));
    printf("device %s, %d compute units\n", prop.gcnArchName, total);
    const int words = (total + 31) / 32;
    if (words > MAX_WORDS) { printf("more compute units than the probe handles\n"); return 2; }
    CK(hipMalloc(&d_where, 2 * WHERE_BLOCKS * sizeof(unsigned)));
    CK(hipMalloc(&d_valu, (size_t)VALU_BLOCKS * 256 * sizeof(float)));
    CK(hipEventCreate(&ev0));
    CK(hipEventCreate(&ev1));
    int bad = 0;
    float ms = 0.f;

    // 3. no mask: the compute units every XCD has
    int own[OV2_CU_MASK_XCDS];
    {
        hipStream_t st;
        CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const std::set<cu_id> seen = run_on(st, &ms);
        per_xcd(seen, own);
        printf("no mask          : %3zu compute units seen, per XCD", seen.size());
        for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) printf(" %d", own[x]);
        printf(", VALU loop %.3f ms\n", ms);
        CK(hipStreamDestroy(st));
    }

    // What a mask must do, per XCD: bit k belongs to XCD k % OV2_CU_MASK_XCDS; an XCD runs on as many compute units as it has
    // bits -- and on ALL of its compute units when it has none (the rule the first run of this probe found: a mask
    // confines an XCD only where it names at least one of its compute units).
    auto check = [&](const uint32_t *mask, const std::set<cu_id> &seen, int cnt[OV2_CU_MASK_XCDS], bool *unconfined) {
        int bits[OV2_CU_MASK_XCDS] = {0};
        for (int k = 0; k < total; ++k)
            if (mask[k >> 5] >> (k & 31) & 1u) ++bits[k % OV2_CU_MASK_XCDS];
        per_xcd(seen, cnt);
        bool ok = true;
        *unconfined = false;
        for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) {
            if (!bits[x]) *unconfined = true;
            ok = ok && cnt[x] == (bits[x] ? bits[x] : own[x]);
        }
        return ok;
    };

    // 1. single bits
    std::vector<int> bits;
    for (int k = 0; k < 16 && k < total; ++k) bits.push_back(k);
    bits.push_back(total - 1);
    for (int k : bits) {
        uint32_t mask[MAX_WORDS] = {0};
        mask[k >> 5] = 1u << (k & 31);
        hipStream_t st;
        CK(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask));
        const std::set<cu_id> seen = run_on(st, &ms);
        int cnt[OV2_CU_MASK_XCDS];
        bool unconfined;
        const bool ok = check(mask, seen, cnt, &unconfined);
        printf("bit %3d          : per XCD", k);
        for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) printf(" %d", cnt[x]);
        printf("; in XCD %d:", k % OV2_CU_MASK_XCDS);
        for (const cu_id &c : seen)
            if (c.xcd == k % OV2_CU_MASK_XCDS) printf(" (SE %d, SH %d, CU %d)", c.se, c.sh, c.cu);
        printf("%s\n", ok ? "" : "   <-- not one compute unit of XCD k % 8 beside whole other XCDs");
        if (!ok) ++bad;
        CK(hipStreamDestroy(st));
    }

    // 2. the builder's masks
    const int ns[4] = {8, 32, 64, 128};
    for (int layout = 0; layout < 2; ++layout)
        for (int n : ns) {
            if (n >= total) continue;
            uint32_t mask[MAX_WORDS] = {0}, back[MAX_WORDS] = {0};
            if (ov2_cu_mask_build(total, n, layout, mask) != OV2_OK) { printf("ov2_cu_mask_build(%d, %d, %d) failed\n", total, n, layout); return 2; }
            hipStream_t st;
            CK(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask));
            CK(hipExtStreamGetCUMask(st, (uint32_t)words, back));
            const std::set<cu_id> seen = run_on(st, &ms);
            int cnt[OV2_CU_MASK_XCDS];
            bool unconfined;
            const bool same = std::equal(mask, mask + words, back);
            const bool ok = check(mask, seen, cnt, &unconfined) && same;
            printf("%s n = %3d  : mask", layout ? "packed" : "spread", n);
            for (int w = 0; w < words; ++w) printf(" %08x", mask[w]);
            printf(", reported back %s, %3zu compute units seen, per XCD", same ? "equal" : "DIFFERENT", seen.size());
            for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) printf(" %d", cnt[x]);
            printf(", VALU loop %.3f ms (x compute units seen = %.1f)%s%s\n", ms, ms * seen.size(),
                   unconfined ? "   [XCDs without a bit: NOT confined to n]" : "", ok ? "" : "   <-- not what the rule says");
            if (!ok) ++bad;
            CK(hipStreamDestroy(st));
        }
    CK(hipFree(d_where));
    CK(hipFree(d_valu));
    printf(bad ? "%d mask(s) NOT honoured\n" : "every mask honoured: an XCD runs on the compute units its bits name, on all of its own when it has no bit\n", bad);
    return bad ? 1 : 0;
}
