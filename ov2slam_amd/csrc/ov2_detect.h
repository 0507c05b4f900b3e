// ov2_detect.h -- what the grid detectors (detect.hip) and the whole-image FAST detector (fastnms.hip) share:
// the span table of cv::circle's filled disc and OpenCV's FAST-9/16 corner score.
#pragma once
#include <hip/hip_runtime.h>

#define DET_MAX_R 16

struct disc_shape {
    int r;
    signed char hw[2 * DET_MAX_R + 1];   // half-width of row offset dy+r of cv::circle's filled midpoint circle
};

inline disc_shape make_disc(int radius)
{   // drawing.cpp Circle(): spans (cy+-dy: +-dx) and (cy+-dx: +-dy)
    disc_shape s;
    s.r = radius;
    for (int i = 0; i < 2 * DET_MAX_R + 1; ++i) s.hw[i] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        auto upd = [&](int row, int half) {
            if (s.hw[radius + row] < half) s.hw[radius + row] = (signed char)half;
            if (s.hw[radius - row] < half) s.hw[radius - row] = (signed char)half;
        };
        upd(dy, dx);
        upd(dx, dy);
        dy++;
        err += plus;
        plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m;
        dx += m;
        minus -= m & 2;
    }
    return s;
}

// FAST-9/16 score of the centre pixel p (cornerScore<16>); 0 when not a corner at `threshold`
__device__ inline int fast_score(const unsigned char *p, int stride, int threshold)
{
    const int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    const int oy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int v = p[0];
    int d[25];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = v - p[oy[k] * stride + ox[k]];
#pragma unroll
    for (int k = 16; k < 25; ++k) d[k] = d[k - 16];
    unsigned br = 0, dk = 0;   // bit k: ring pixel k brighter / darker than the centre by more than the threshold
#pragma unroll
    for (int k = 0; k < 16; ++k) { br |= (d[k] < -threshold ? 1u : 0u) << k; dk |= (d[k] > threshold ? 1u : 0u) << k; }
    br |= br << 16; dk |= dk << 16;
    bool corner = false;
#pragma unroll
    for (int s = 0; s < 16; ++s) corner |= (((br >> s) & 0x1ffu) == 0x1ffu) | (((dk >> s) & 0x1ffu) == 0x1ffu);
    if (!corner) return 0;
    int a0 = threshold;
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        int a = min(min(d[k + 1], d[k + 2]), d[k + 3]);
        if (a <= a0) continue;
        a = min(a, min(min(d[k + 4], d[k + 5]), min(min(d[k + 6], d[k + 7]), d[k + 8])));
        a0 = max(a0, min(a, d[k]));
        a0 = max(a0, min(a, d[k + 9]));
    }
    int b0 = -a0;
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        int b = max(max(d[k + 1], d[k + 2]), max(d[k + 3], max(d[k + 4], d[k + 5])));
        if (b >= b0) continue;
        b = max(b, max(d[k + 6], max(d[k + 7], d[k + 8])));
        b0 = min(b0, max(b, d[k]));
        b0 = min(b0, max(b, d[k + 9]));
    }
    return -b0 - 1;
}
