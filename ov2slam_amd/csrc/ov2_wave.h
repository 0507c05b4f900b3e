// ov2_wave.h -- the fixed-order wave / workgroup reductions of the kernels, written once.  Every sum that has to round
// like the oracle's is a tree of a fixed shape, so the shape lives here: DPP moves inside a row of 16 lanes, readlane
// across the four rows of a wave, LDS across the waves of a 256-thread workgroup.  The two-smallest-keys reduction of the
// descriptor matcher uses the same moves.  The border index that the image kernels share stands at the end.
#pragma once
#include <hip/hip_runtime.h>

namespace ov2wave {

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// the bare move: lanes whose source lane does not exist read 0 (bound_ctrl), so no register has to be zeroed for them first
template <int CTRL>
__device__ __forceinline__ int dpp_mov_i32(int v)
{
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)dpp_i32<CTRL>((int)(b & 0xffffffffll));
    const unsigned hi = (unsigned)dpp_i32<CTRL>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | lo);
}

__device__ __forceinline__ double readlane_f64(double v, int lane)   // lane must be wave-uniform
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | lo);
}

// Sum over the GW (8 | 16) lanes of a lane group inside a DPP row, total in every lane of the group: the pairwise tree
// ((l0+l1)+(l2+l3))+...  After the two quad steps all lanes of a quad agree, so the mirror steps pair equal partial sums
// exactly like xor 4 / xor 8 would.
template <int GW>
__device__ __forceinline__ double row_sum_f64(double v)
{
    static_assert(GW == 8 || GW == 16, "a lane group is half a DPP row or a whole one");
    v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);   // row_half_mirror: lane l <-> 7 - l of its half row
    if (GW == 16) v += dpp_f64<0x140>(v);   // row_mirror
    return v;
}

template <int GW>
__device__ __forceinline__ int row_sum_i32(int v)
{
    static_assert(GW == 8 || GW == 16, "a lane group is half a DPP row or a whole one");
    v += dpp_i32<0xB1>(v);
    v += dpp_i32<0x4E>(v);
    v += dpp_i32<0x141>(v);
    if (GW == 16) v += dpp_i32<0x140>(v);
    return v;
}

// sum over the 64 lanes of a wave, wave-uniform: the four row sums in the fixed order (l0 + l16) + (l32 + l48)
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v = row_sum_f64<16>(v);
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// The two smallest of the keys that the GW (4 | 16) lanes of a lane group inside a DPP row hold, two per lane (lo <= hi), to
// every lane of the group.  Exact and order-free as long as the keys of a group are distinct (a filler above every key, such
// as INT_MAX, may repeat): the smallest of a union is the smaller of the two lows, the second the smaller of the larger
// low and the two highs.  Each step pairs disjoint sets of lanes (after the quad steps a quad agrees).
__device__ __forceinline__ void min2_merge_i32(int &lo, int &hi, int olo, int ohi)
{
    hi = min(max(lo, olo), min(hi, ohi));
    lo = min(lo, olo);
}

template <int GW>
__device__ __forceinline__ void row_min2_i32(int &lo, int &hi)
{
    static_assert(GW == 4 || GW == 16, "a lane group is a quad or a whole DPP row");
    min2_merge_i32(lo, hi, dpp_i32<0xB1>(lo), dpp_i32<0xB1>(hi));
    min2_merge_i32(lo, hi, dpp_i32<0x4E>(lo), dpp_i32<0x4E>(hi));
    if (GW == 16) {
        min2_merge_i32(lo, hi, dpp_i32<0x141>(lo), dpp_i32<0x141>(hi));
        min2_merge_i32(lo, hi, dpp_i32<0x140>(lo), dpp_i32<0x140>(hi));
    }
}

// the same over the 64 lanes of a wave, wave-uniform: the four rows merged as (l0, l16), (l32, l48)
__device__ __forceinline__ void wave_min2_i32(int &lo, int &hi)
{
    row_min2_i32<16>(lo, hi);
    int alo = __builtin_amdgcn_readlane(lo, 0), ahi = __builtin_amdgcn_readlane(hi, 0);
    min2_merge_i32(alo, ahi, __builtin_amdgcn_readlane(lo, 16), __builtin_amdgcn_readlane(hi, 16));
    int blo = __builtin_amdgcn_readlane(lo, 32), bhi = __builtin_amdgcn_readlane(hi, 32);
    min2_merge_i32(blo, bhi, __builtin_amdgcn_readlane(lo, 48), __builtin_amdgcn_readlane(hi, 48));
    min2_merge_i32(alo, ahi, blo, bhi);
    lo = alo; hi = ahi;
}

// Ordered sum of one double per thread of a 256-thread workgroup through sh[256], total to every thread.  No barrier
// behind the last read of sh[0]: a caller that writes sh again before its next barrier puts a __syncthreads() first.
__device__ inline double block_sum_256(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// Raises the calling wave to priority `level` (0..3; 0 issues nothing) for the rest of its life.  s_setprio takes an
// immediate and ignores EXEC, so the level is forced wave-uniform first and the choice among the three instructions is
// made by scalar compares and branches: a guard lowered through EXEC would run every s_setprio it guards.
__device__ __forceinline__ void set_wave_prio(int level)
{
    const int l = __builtin_amdgcn_readfirstlane(level);
    if (l == 1) __builtin_amdgcn_s_setprio(1);
    else if (l == 2) __builtin_amdgcn_s_setprio(2);
    else if (l == 3) __builtin_amdgcn_s_setprio(3);
}

// cv::BORDER_REFLECT_101 index; one reflection is enough for |overshoot| < n (callers guarantee it)
__device__ __forceinline__ int reflect101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

}  // namespace ov2wave
