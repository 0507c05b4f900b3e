// sac_common.h -- what the sample-consensus stages (epipolar.hip: 5-point RANSAC, p3p.hip: P3P LMedS / RANSAC) share:
// the seeded counter sampler documented at ov2_epipolar_filter_batch (include/ov2slam_hip.h) and OpenGV's RANSAC
// iteration bound.  Host + device, so that a CPU build of a stage can be compared with the kernels.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef HD
#define HD __host__ __device__
#endif

// ---- sampler: SplitMix64 finaliser, draw d / attempt j of a frame's stream, multiply-shift reduction to [0, n) ----
HD inline uint64_t epi_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HD inline uint32_t epi_hash(uint64_t seed, uint32_t d, uint32_t j, uint32_t n)
{
    const uint64_t a = epi_mix(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)d + 1));
    const uint64_t x = epi_mix(a + 0x9E3779B97F4A7C15ull * ((uint64_t)j + 1));
    return (uint32_t)(((x >> 32) * (uint64_t)n) >> 32);
}
// S distinct indices of [0, n), n >= S: attempt j = 0, 1, ...; a duplicate is redrawn; after 256 attempts the
// smallest unused index is taken (never reached for n >= 8 in practice, keeps the worst case bounded)
template <int S>
HD inline void sac_draw(uint64_t seed, int d, int n, int *idx)
{
    uint32_t j = 0;
    for (int s = 0; s < S; ++s) {
        int v = -1;
        while (v < 0 && j < 256) {
            const int c = (int)epi_hash(seed, (uint32_t)d, j++, (uint32_t)n);
            bool dup = false;
            for (int q = 0; q < s; ++q) dup = dup || idx[q] == c;
            if (!dup) v = c;
        }
        for (int c = 0; c < n && v < 0; ++c) {
            bool dup = false;
            for (int q = 0; q < s; ++q) dup = dup || idx[q] == c;
            if (!dup) v = c;
        }
        idx[s] = v;
    }
}

// OpenGV Ransac::computeModel, probability 0.99: the iteration bound k after a model with `best` of n inliers
HD inline double sac_ransac_k(int best, int n, double sample_size)
{
    const double w = (double)best / (double)n;
    double pno = 1.0 - pow(w, sample_size);
    pno = fmax(2.220446049250313e-16, pno);
    pno = fmin(1.0 - 2.220446049250313e-16, pno);
    return log(1.0 - 0.99) / log(pno);
}

// ---- real roots of a polynomial (coefficients ascending), bounded work ----
// p(z) and p'(z)
HD inline double peval(const double *p, int n, double z, double *dp)
{
    double v = p[n], d = 0.;
    for (int i = n - 1; i >= 0; --i) { d = d * z + v; v = v * z + p[i]; }
    *dp = d;
    return v;
}

// the single root of a polynomial that is monotone on [lo, hi] and changes sign there (safeguarded Newton)
HD inline double root_bracket(const double *p, int n, double lo, double hi, double flo)
{
    double x = 0.5 * (lo + hi);
    for (int it = 0; it < 200; ++it) {
        double df;
        const double f = peval(p, n, x, &df);
        if (f == 0.) return x;
        if ((f < 0.) == (flo < 0.)) lo = x; else hi = x;
        double xn = x - f / df;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        if (hi - lo <= 4e-16 * fabs(x) || xn == x) return xn;
        x = xn;
    }
    return x;
}

// real roots of p (degree n, p[n] != 0) inside [lo, hi] into cp, ascending: the roots of p^(k) there are isolated between
// consecutive roots of p^(k+1) (k = n-1 .. 0) and the two ends.  q (n + 1), cp (n) and nr (n) are the caller's workspace.
HD inline int sac_real_roots_in(const double *p, int n, double lo, double hi, double *q, double *cp, double *nr)
{
    int ncp = 0;
    for (int k = n - 1; k >= 0; --k) {
        const int deg = n - k;
        for (int i = 0; i <= deg; ++i) {   // q = p^(k)
            double f = 1.;
            for (int m = 0; m < k; ++m) f *= (double)(i + k - m);
            q[i] = p[i + k] * f;
        }
        int m = 0;
        for (int s = 0; s <= ncp; ++s) {
            const double a = s == 0 ? lo : cp[s - 1], b = s == ncp ? hi : cp[s];
            double dd;
            const double fa = peval(q, deg, a, &dd), fb = peval(q, deg, b, &dd);
            if (fb == 0.) { nr[m++] = b; continue; }
            if (fa == 0. || (fa < 0.) == (fb < 0.)) continue;
            nr[m++] = root_bracket(q, deg, a, b, fa);
        }
        for (int i = 0; i < m; ++i) cp[i] = nr[i];
        ncp = m;
    }
    return ncp;
}

// all real roots: inside the Cauchy bound
HD inline int sac_real_roots(const double *p, int n, double *q, double *cp, double *nr)
{
    double bound = 0.;
    for (int i = 0; i < n; ++i) bound = fmax(bound, fabs(p[i] / p[n]));
    bound += 1.;
    return sac_real_roots_in(p, n, -bound, bound, q, cp, nr);
}
