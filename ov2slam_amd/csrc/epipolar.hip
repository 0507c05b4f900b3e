// epipolar.hip -- the per-frame 2D-2D epipolar filter on gfx950: batched 5-point RANSAC + the Sampson gate.
//
// Replaces (reference): VisualFrontEnd::epipolar2d2dFiltering src/visual_front_end.cpp:446-655 from the
// compute5ptEssentialMatrix call (:557) on, i.e. MultiViewGeometry::opengv5ptEssentialMatrix
// src/multi_view_geometry.cpp:594-697 (OpenGV sac::Ransac<CentralRelativePoseSacProblem>, algorithm NISTER) and the
// stereo gate :611-648 (computeFundamentalMat12 :824-838, computeSampsonDistance :798-813).  OpenGV is an un-vendored
// dependency; what is restated here is its published source and Nister's paper (PAMI 26(6), 2004):
//   * Ransac::computeModel, probability 0.99: while (iterations < k && skipped < 10 max_iter) { draw 5; model fails ->
//     ++skipped, continue; count = #(score < th); if count > best (best starts at -INT_MAX): best = count,
//     k = log(0.01) / log(clamp(1 - (best / N)^5, eps, 1 - eps)); ++iterations; if iterations > max_iter break }.
//     Inliers = pairs with score < th under the best model, outliers = the complement.
//   * the 5-point model: null space of the 5 x 9 epipolar rows (Householder QR), Nister's 10 x 20 cubic system
//     (det E = 0, 2 E E^T E - tr(E E^T) E = 0) reduced by Gauss-Jordan, the 3 x 3 polynomial matrix in z, its degree-10
//     determinant, real roots, (x, y) from the null vector.  Each E gives four (R, t) candidates (the twisted pair times
//     +-t); the one with the lowest summed score over the 5 sample points is kept.  No real root -> the draw is skipped.
//   * score of a pair under (R, t): triangulate2 (OpenGV's mid-point method, as tri.hip), reproject into both views,
//     normalise, (1 - f1.r1) + (1 - f2.r2).  th = 2 (1 - cos(atan(errth / focal))), focal = (fx + fy) / 2 in float.
// Deviations (parity section):
//   * the sampler: draw d takes its 5 distinct indices from epi_hash(seed, d, j), j = 0, 1, ... (redraw on a duplicate);
//     the reference seeds OpenGV from the clock.  Draws are independent, so a round of EPI_ROUND draws runs in parallel
//     and OpenGV's loop is then replayed over the round's (ok, count) results in draw order.
//   * candidate ties: every E fits its own 5 points exactly, so two valid E of one sample differ in summed score only by
//     rounding noise.  Candidates within 1e-9 of the lowest score are broken by the larger trace of R (the smaller
//     rotation), so the pick does not depend on root order or rounding.
//   * t is returned as a unit vector (OpenGV returns sigma1 U_3, a scale that depends on the null-space basis).
// Mapping: one 256-thread workgroup per frame.  A round solves EPI_ROUND draws, one lane each (f64, serial, on a
// workspace in LDS: no kernel here uses scratch), then the
// whole workgroup scores the round's models over the frame's pairs (read from global memory; L2-resident across
// rounds) with exact integer counts, and one lane replays OpenGV's loop.  A launch evaluates at most 11 max_iter + 1 draws.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ov2_internal.h"

#define HD __host__ __device__
#include "sac_common.h"   // the sampler (epi_hash, sac_draw) and OpenGV's iteration bound

namespace {

enum { EPI_THREADS = 256, EPI_ROUND = 16, FIVEPT_THREADS = 16, K_EPI = OV2_K_MAP + 7, K_FIVEPT = OV2_K_MAP + 8 };

HD inline double epi_sqrt(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

// ---- score of one pair (OpenGV getSelectedDistancesToModel: triangulate2 + normalised reprojections) ----
HD inline double epi_score(const double R[9], const double t[3], const double f1[3], const double f2[3])
{
    const double f2u[3] = {R[0] * f2[0] + R[1] * f2[1] + R[2] * f2[2], R[3] * f2[0] + R[4] * f2[1] + R[5] * f2[2],
                           R[6] * f2[0] + R[7] * f2[1] + R[8] * f2[2]};
    const double a00 = f1[0] * f1[0] + f1[1] * f1[1] + f1[2] * f1[2];
    const double a10 = f1[0] * f2u[0] + f1[1] * f2u[1] + f1[2] * f2u[2];
    const double a01 = -a10;
    const double a11 = -(f2u[0] * f2u[0] + f2u[1] * f2u[1] + f2u[2] * f2u[2]);
    const double b0 = t[0] * f1[0] + t[1] * f1[1] + t[2] * f1[2];
    const double b1 = t[0] * f2u[0] + t[1] * f2u[1] + t[2] * f2u[2];
    const double invdet = 1. / (a00 * a11 - a01 * a10);
    const double l0 = (a11 * invdet) * b0 + (-a01 * invdet) * b1;
    const double l1 = (-a10 * invdet) * b0 + (a00 * invdet) * b1;
    double X[3];
    for (int k = 0; k < 3; ++k) X[k] = (l0 * f1[k] + (t[k] + l1 * f2u[k])) / 2.;
    // inverse transformation [R^T | -R^T t] applied to [X; 1]
    const double ti[3] = {-(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]),
                          -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])};
    const double Xb[3] = {R[0] * X[0] + R[3] * X[1] + R[6] * X[2] + ti[0], R[1] * X[0] + R[4] * X[1] + R[7] * X[2] + ti[1],
                          R[2] * X[0] + R[5] * X[1] + R[8] * X[2] + ti[2]};
    const double n1 = epi_sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    const double n2 = epi_sqrt(Xb[0] * Xb[0] + Xb[1] * Xb[1] + Xb[2] * Xb[2]);
    const double r1[3] = {X[0] / n1, X[1] / n1, X[2] / n1}, r2[3] = {Xb[0] / n2, Xb[1] / n2, Xb[2] / n2};
    const double e1 = 1.0 - (f1[0] * r1[0] + f1[1] * r1[1] + f1[2] * r1[2]);
    const double e2 = 1.0 - (f2[0] * r2[0] + f2[1] * r2[1] + f2[2] * r2[2]);
    return e1 + e2;
}

// ---- Nister's 5-point solver ----
// Every array the solver indexes at run time lives in a per-lane workspace (LDS in the kernels), so that no kernel needs
// scratch memory; what stays in registers is indexed by constants only.
// polynomials in (x, y, z): linear over (x, y, z, 1); quadratic over the pairs a <= b of that basis (10);
// cubic in Nister's column order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
struct epi_ws {
    double N[4][9];        // null-space basis X, Y, Z, W: E = x X + y Y + z Z + W
    double M[10][20];      // the 10 cubic constraints, then their Gauss-Jordan form
    union {
        struct { double A[9][5], V[5][9], beta[5]; } qr;               // Householder QR of Q^T
        double EE[6][10];                                              // E E^T (upper triangle), quadratics
        struct { double P[3][3][5], p[11], q[11], cp[10], nr[10]; } rt;   // polynomial matrix, det, root cascade
    } u;
    double Es[10][9];      // solutions
    double f1[5][3], f2[5][3];
    int idx[5];
};

HD constexpr int mono3(int a, int b, int c)   // exponents of x, y, z (a + b + c <= 3)
{
    return a == 3 ? 0 : b == 3 ? 1 : (a == 2 && b == 1) ? 2 : (a == 1 && b == 2) ? 3 : (a == 2 && c == 1) ? 4 : a == 2 ? 5
         : (b == 2 && c == 1) ? 6 : b == 2 ? 7 : (a == 1 && b == 1 && c == 1) ? 8 : (a == 1 && b == 1) ? 9
         : (a == 1 && c == 2) ? 10 : (a == 1 && c == 1) ? 11 : a == 1 ? 12 : (b == 1 && c == 2) ? 13 : (b == 1 && c == 1) ? 14
         : b == 1 ? 15 : c == 3 ? 16 : c == 2 ? 17 : c == 1 ? 18 : 19;
}
HD constexpr int pidx(int a, int b) { return a == 0 ? b : a == 1 ? 3 + b : a == 2 ? 5 + b : 9; }   // a <= b < 4
HD constexpr int ex(int i, int v) { return i == v ? 1 : 0; }
HD constexpr int cidx(int a, int b, int c)
{
    return mono3(ex(a, 0) + ex(b, 0) + ex(c, 0), ex(a, 1) + ex(b, 1) + ex(c, 1), ex(a, 2) + ex(b, 2) + ex(c, 2));
}
HD constexpr int eidx(int i, int j) { return i <= j ? (i == 0 ? j : i == 1 ? 2 + j : 5) : (j == 0 ? i : j == 1 ? 2 + i : 5); }

// linear poly of entry e of E: coefficients of x, y, z, 1
HD inline void lin(const epi_ws &w, int e, double l[4])
{
    l[0] = w.N[0][e]; l[1] = w.N[1][e]; l[2] = w.N[2][e]; l[3] = w.N[3][e];
}
HD inline void pmul11(const double l[4], const double m[4], double q[10])
{
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) q[pidx(a, b)] = a == b ? l[a] * m[a] : l[a] * m[b] + l[b] * m[a];
}
HD inline void pmul21_acc(const double q[10], const double l[4], double s, double *c)
{
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) c[cidx(a, b, k)] += s * (q[pidx(a, b)] * l[k]);
}

// real roots of w.u.rt.p (degree n <= 10, p[n] != 0) into w.u.rt.cp, ascending (sac_common.h)
HD inline int real_roots(epi_ws &w, int n) { return sac_real_roots(w.u.rt.p, n, w.u.rt.q, w.u.rt.cp, w.u.rt.nr); }

// Gauss-Newton on the 10 cubic constraints (2 E E^T E - tr(E E^T) E = 0, det E = 0) in the homogeneous coefficients
// v of E = v0 X + v1 Y + v2 Z + v3 W, |v| = 1 (steps orthogonal to v): the degree-10 reduction loses digits on some
// samples, most where a root is large.  At most 9 steps; a step that does not lower the residual is undone.  The
// working matrices go to w.M, dead once the polynomial matrix is built (few registers: no spills).
HD inline double polish_v(epi_ws &w, double v[4])   // returns the squared residual at v
{
    double *J = &w.M[0][0], *E = J + 40, *EEt = E + 9, *EtE = EEt + 9, *C = EtE + 9, *r = C + 9;   // J: 10 x 4
    double prev = INFINITY, sv[4] = {v[0], v[1], v[2], v[3]};
#pragma nounroll
    for (int it = 0; it < 10; ++it) {
#pragma nounroll
        for (int e = 0; e < 9; ++e) E[e] = v[0] * w.N[0][e] + v[1] * w.N[1][e] + v[2] * w.N[2][e] + v[3] * w.N[3][e];
#pragma nounroll
        for (int i = 0; i < 3; ++i)
#pragma nounroll
            for (int j = 0; j < 3; ++j) {
                EEt[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
                EtE[3 * i + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
                const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                C[3 * i + j] = E[3 * i1 + j1] * E[3 * i2 + j2] - E[3 * i1 + j2] * E[3 * i2 + j1];
            }
        const double tr = EEt[0] + EEt[4] + EEt[8];
        double rr = 0.;
#pragma nounroll
        for (int i = 0; i < 3; ++i)
#pragma nounroll
            for (int j = 0; j < 3; ++j) {
                const double x = 2. * (EEt[3 * i] * E[j] + EEt[3 * i + 1] * E[3 + j] + EEt[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
                r[3 * i + j] = x;
                rr += x * x;
            }
        r[9] = E[0] * C[0] + E[1] * C[1] + E[2] * C[2];
        rr += r[9] * r[9];
        if (!(rr < prev)) { for (int k = 0; k < 4; ++k) v[k] = sv[k]; return prev; }
        if (rr == 0. || it == 9) return rr;
        prev = rr;
        for (int k = 0; k < 4; ++k) sv[k] = v[k];
#pragma nounroll
        for (int c = 0; c < 4; ++c) {   // directional derivatives along X, Y, Z, W
            const double *D = w.N[c];
            double ed = 0., dd = 0.;
#pragma nounroll
            for (int e = 0; e < 9; ++e) { ed += E[e] * D[e]; dd += C[e] * D[e]; }
#pragma nounroll
            for (int i = 0; i < 3; ++i)
#pragma nounroll
                for (int j = 0; j < 3; ++j) {
                    double t1 = 0., t2 = 0., t3 = 0.;
#pragma nounroll
                    for (int k = 0; k < 3; ++k) {
                        t1 += D[3 * i + k] * EtE[3 * k + j];                                   // D E^T E
                        const double dte = D[k] * E[j] + D[3 + k] * E[3 + j] + D[6 + k] * E[6 + j];   // (D^T E)_kj
                        t2 += E[3 * i + k] * dte;                                              // E D^T E
                        t3 += EEt[3 * i + k] * D[3 * k + j];                                   // E E^T D
                    }
                    J[4 * (3 * i + j) + c] = 2. * (t1 + t2 + t3) - tr * D[3 * i + j] - 2. * ed * E[3 * i + j];
                }
            J[36 + c] = dd;
        }
        // (J^T J + v v^T) dv = -J^T r: Cholesky of the 4 x 4 system
        double A[4][4], g[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            g[a] = 0.;
#pragma unroll
            for (int b = 0; b < 4; ++b) A[a][b] = v[a] * v[b];
        }
#pragma nounroll
        for (int e = 0; e < 10; ++e) {
            const double j0 = J[4 * e], j1 = J[4 * e + 1], j2 = J[4 * e + 2], j3 = J[4 * e + 3], re = r[e];
            const double jj[4] = {j0, j1, j2, j3};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                g[a] -= jj[a] * re;
#pragma unroll
                for (int b = 0; b < 4; ++b) A[a][b] += jj[a] * jj[b];
            }
        }
        bool okc = true;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < a; ++b) {
                double sum = A[a][b];
#pragma unroll
                for (int k = 0; k < b; ++k) sum -= A[a][k] * A[b][k];
                A[a][b] = sum / A[b][b];
            }
            double d = A[a][a];
#pragma unroll
            for (int k = 0; k < a; ++k) d -= A[a][k] * A[a][k];
            okc = okc && d > 0.;
            A[a][a] = epi_sqrt(d > 0. ? d : 1.);
        }
        if (!okc) return rr;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double sum = g[a];
#pragma unroll
            for (int k = 0; k < a; ++k) sum -= A[a][k] * g[k];
            g[a] = sum / A[a][a];
        }
#pragma unroll
        for (int a = 3; a >= 0; --a) {
            double sum = g[a];
#pragma unroll
            for (int k = a + 1; k < 4; ++k) sum -= A[k][a] * g[k];
            g[a] = sum / A[a][a];
        }
        double nv = 0.;
#pragma unroll
        for (int a = 0; a < 4; ++a) { v[a] += g[a]; nv += v[a] * v[a]; }
        nv = epi_sqrt(nv);
        if (!(nv > 0. && nv < INFINITY)) { for (int k = 0; k < 4; ++k) v[k] = sv[k]; return rr; }
#pragma unroll
        for (int a = 0; a < 4; ++a) v[a] /= nv;
    }
    return prev;
}

// up to 10 essential matrices E (w.Es, row-major, ||E||_F = 1) with f1_i^T E f2_i = 0 for the 5 pairs w.f1, w.f2
HD inline int fivept_nister(epi_ws &w)
{
    // null space of the 5 x 9 rows q_i = vec(f1_i f2_i^T): Householder QR of Q^T (9 x 5)
    auto &A = w.u.qr.A;
    auto &V = w.u.qr.V;
    auto &beta = w.u.qr.beta;
    for (int i = 0; i < 5; ++i)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) A[3 * a + b][i] = w.f1[i][a] * w.f2[i][b];
    for (int j = 0; j < 5; ++j) {
        double nrm2 = 0.;
        for (int r = j; r < 9; ++r) nrm2 += A[r][j] * A[r][j];
        const double nrm = epi_sqrt(nrm2);
        const double alpha = A[j][j] >= 0. ? -nrm : nrm;
        for (int r = 0; r < 9; ++r) V[j][r] = r < j ? 0. : A[r][j];
        V[j][j] -= alpha;
        double vn2 = 0.;
        for (int r = j; r < 9; ++r) vn2 += V[j][r] * V[j][r];
        beta[j] = vn2 > 0. ? 2. / vn2 : 0.;
        for (int c = j; c < 5; ++c) {
            double s = 0.;
            for (int r = j; r < 9; ++r) s += V[j][r] * A[r][c];
            s *= beta[j];
            for (int r = j; r < 9; ++r) A[r][c] -= s * V[j][r];
        }
    }
    for (int k = 0; k < 4; ++k) {   // N_k = H_0 .. H_4 e_{5+k}
        double *e = w.N[k];
        for (int r = 0; r < 9; ++r) e[r] = r == 5 + k ? 1. : 0.;
        for (int j = 4; j >= 0; --j) {
            double s = 0.;
            for (int r = j; r < 9; ++r) s += V[j][r] * e[r];
            s *= beta[j];
            for (int r = j; r < 9; ++r) e[r] -= s * V[j][r];
        }
    }
    // E E^T (symmetric, 6 quadratics), tr, then the rows of 2 E E^T E - tr E and det E
    auto &EE = w.u.EE;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double l[4], m[4], q[10];
                lin(w, 3 * i + k, l);
                lin(w, 3 * j + k, m);
                pmul11(l, m, q);
#pragma unroll
                for (int u = 0; u < 10; ++u) acc[u] += q[u];
            }
#pragma unroll
            for (int u = 0; u < 10; ++u) EE[eidx(i, j)][u] = acc[u];
        }
    for (int r = 0; r < 10; ++r)
        for (int c = 0; c < 20; ++c) w.M[r][c] = 0.;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) {
                double q[10], l[4];
#pragma unroll
                for (int u = 0; u < 10; ++u)
                    q[u] = 2. * EE[eidx(i, k)][u] - (i == k ? EE[0][u] + EE[3][u] + EE[5][u] : 0.);
                lin(w, 3 * k + j, l);
                pmul21_acc(q, l, 1., w.M[3 * i + j]);
            }
    {   // det E by the first row
        double q[10], l0[4], l1[4], l2[4], a[4], b[4];
        lin(w, 0, l0); lin(w, 1, l1); lin(w, 2, l2);
        lin(w, 4, a); lin(w, 8, b); pmul11(a, b, q); pmul21_acc(q, l0, 1., w.M[9]);
        lin(w, 5, a); lin(w, 7, b); pmul11(a, b, q); pmul21_acc(q, l0, -1., w.M[9]);
        lin(w, 3, a); lin(w, 8, b); pmul11(a, b, q); pmul21_acc(q, l1, -1., w.M[9]);
        lin(w, 5, a); lin(w, 6, b); pmul11(a, b, q); pmul21_acc(q, l1, 1., w.M[9]);
        lin(w, 3, a); lin(w, 7, b); pmul11(a, b, q); pmul21_acc(q, l2, 1., w.M[9]);
        lin(w, 4, a); lin(w, 6, b); pmul11(a, b, q); pmul21_acc(q, l2, -1., w.M[9]);
    }
    // Gauss-Jordan on the first 10 columns, partial pivoting
    auto &M = w.M;
    for (int c = 0; c < 10; ++c) {
        int piv = c;
        for (int r = c + 1; r < 10; ++r)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (!(fabs(M[piv][c]) > 0.)) return 0;
        if (piv != c)
            for (int u = 0; u < 20; ++u) { const double tmp = M[c][u]; M[c][u] = M[piv][u]; M[piv][u] = tmp; }
        const double inv = 1. / M[c][c];
        for (int u = c; u < 20; ++u) M[c][u] *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = M[r][c];
            if (f == 0.) continue;
            for (int u = c; u < 20; ++u) M[r][u] -= f * M[c][u];
        }
    }
    // <k> = <x^2z> - z <x^2>, <l> = <y^2z> - z <y^2>, <m> = <xyz> - z <xy>: rows x (deg 3), y (deg 3), 1 (deg 4) in z
    auto &P = w.u.rt.P;
    for (int e = 0; e < 3; ++e) {
        const double *a = &M[4 + 2 * e][10], *b = &M[5 + 2 * e][10];   // tails over xz^2 xz x yz^2 yz y z^3 z^2 z 1
        for (int v = 0; v < 2; ++v) {
            const double *ta = a + 3 * v, *tb = b + 3 * v;
            P[e][v][3] = -tb[0]; P[e][v][2] = ta[0] - tb[1]; P[e][v][1] = ta[1] - tb[2]; P[e][v][0] = ta[2]; P[e][v][4] = 0.;
        }
        P[e][2][4] = -b[6]; P[e][2][3] = a[6] - b[7]; P[e][2][2] = a[7] - b[8]; P[e][2][1] = a[8] - b[9]; P[e][2][0] = a[9];
    }
    // det of the 3 x 3 polynomial matrix: degree 10
    double *p = w.u.rt.p, *m2 = w.u.rt.q;
    for (int i = 0; i < 11; ++i) p[i] = 0.;
    for (int c0 = 0; c0 < 3; ++c0) {
        const int c1 = (c0 + 1) % 3, c2 = (c0 + 2) % 3;
        for (int i = 0; i < 9; ++i) m2[i] = 0.;   // P[1][c1] P[2][c2] - P[1][c2] P[2][c1]
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5 && i + j < 9; ++j) m2[i + j] += P[1][c1][i] * P[2][c2][j] - P[1][c2][i] * P[2][c1][j];
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 9 && i + j < 11; ++j) p[i + j] += P[0][c0][i] * m2[j];
    }
    int n = 10;
    while (n > 0 && p[n] == 0.) --n;
    if (n == 0) return 0;
    const int nr = real_roots(w, n);
    int ns = 0;
    for (int s = 0; s < nr; ++s) {
        double zs = w.u.rt.cp[s];
        double B3[3][3];
        // the root of the expanded degree-10 polynomial, refined by Newton on det B3(z) evaluated directly (the expansion
        // loses digits on some samples); a step that does not lower |det| is not taken
        double fprev = INFINITY;
#pragma nounroll
        for (int it = 0; it < 4; ++it) {
            double dB[3][3];
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int v = 0; v < 3; ++v) B3[e][v] = peval(P[e][v], 4, zs, &dB[e][v]);
            double f = 0., df = 0.;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int v1 = (v + 1) % 3, v2 = (v + 2) % 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int e1 = (e + 1) % 3, e2 = (e + 2) % 3;
                    const double cof = B3[e1][v1] * B3[e2][v2] - B3[e1][v2] * B3[e2][v1];
                    if (e == 0) f += B3[0][v] * cof;
                    df += dB[e][v] * cof;
                }
            }
            if (!(fabs(f) < fprev) || it == 3 || df == 0.) break;
            fprev = fabs(f);
            const double zn = zs - f / df;
            if (!(fabs(zn - zs) <= 1e-3 * (1. + fabs(zs)))) break;
            zs = zn;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                double dd;
                B3[e][v] = peval(P[e][v], 4, zs, &dd);
            }
        // (x, y, 1) spans the null space of B3: the row-pair cross product of the largest norm
        double best = -1., xs = 0., ys = 0.;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double *u = B3[r], *v = B3[(r + 1) % 3];
            const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
            const double nc = cx * cx + cy * cy + cz * cz;
            if (nc > best && cz != 0.) { best = nc; xs = cx / cz; ys = cy / cz; }
        }
        if (!(best > 0.)) continue;
        double v[4] = {xs, ys, zs, 1.};
        const double vn = epi_sqrt(xs * xs + ys * ys + zs * zs + 1.);
        if (!(vn < INFINITY)) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] /= vn;
        if (!(polish_v(w, v) <= 1e-12)) continue;   // not a solution after all (residual > 1e-6 at |v| = 1)
        double E[9], nn = 0.;
#pragma unroll
        for (int e = 0; e < 9; ++e) { E[e] = v[0] * w.N[0][e] + v[1] * w.N[1][e] + v[2] * w.N[2][e] + v[3] * w.N[3][e]; nn += E[e] * E[e]; }
        nn = epi_sqrt(nn);
        if (!(nn > 0.) || !(nn < INFINITY)) continue;
        bool dup = false;   // a root the polish moved onto a solution already found is not a second solution
        for (int q = 0; q < ns && !dup; ++q) {
            double dp = 0., dm = 0.;
            for (int e = 0; e < 9; ++e) { dp = fmax(dp, fabs(w.Es[q][e] - E[e] / nn)); dm = fmax(dm, fabs(w.Es[q][e] + E[e] / nn)); }
            dup = fmin(dp, dm) < 1e-9;
        }
        if (dup) continue;
        for (int e = 0; e < 9; ++e) w.Es[ns][e] = E[e] / nn;
        ++ns;
    }
    return ns;
}

HD inline void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// OpenGV computeModelCoefficients (NISTER): solve, decompose each E into its four (R, t), keep the lowest summed score
// over the sample (ties within 1e-9 -> larger trace of R).  E = [t]x R, ||E||_F^2 = 2, |t| = 1:
// R = Cof(E) - [t]x E and its twin Cof(E) + [t]x E.
HD inline bool epi_model(epi_ws &w, double *Rout, double *tout)
{
    const int ns = fivept_nister(w);
    double bq = INFINITY, btr = -INFINITY;
    bool have = false;
    for (int pass = 0; pass < 2; ++pass)
        for (int s = 0; s < ns; ++s) {
            double E[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) E[e] = w.Es[s][e] * 1.4142135623730951;
            const double c0[3] = {E[0], E[3], E[6]}, c1[3] = {E[1], E[4], E[7]}, c2[3] = {E[2], E[5], E[8]};   // columns
            double x01[3], x12[3], x20[3];
            cross3(c0, c1, x01); cross3(c1, c2, x12); cross3(c2, c0, x20);
            const double n01 = x01[0] * x01[0] + x01[1] * x01[1] + x01[2] * x01[2];
            const double n12 = x12[0] * x12[0] + x12[1] * x12[1] + x12[2] * x12[2];
            const double n20 = x20[0] * x20[0] + x20[1] * x20[1] + x20[2] * x20[2];
            const bool p01 = n01 >= n12 && n01 >= n20, p12 = !p01 && n12 >= n20;
            const double tn = epi_sqrt(p01 ? n01 : p12 ? n12 : n20);
            if (!(tn > 0.)) continue;
            double t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = (p01 ? x01[k] : p12 ? x12[k] : x20[k]) / tn;
            double Ra[9], Rb[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double cof = j == 0 ? x12[i] : j == 1 ? x20[i] : x01[i];
                    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
                    const double txe = t[i1] * E[3 * i2 + j] - t[i2] * E[3 * i1 + j];   // ([t]x E)_ij
                    Ra[3 * i + j] = cof - txe;
                    Rb[3 * i + j] = cof + txe;
                }
#pragma unroll
            for (int cnd = 0; cnd < 4; ++cnd) {
                const double *R = (cnd & 1) ? Rb : Ra;
                const double sg = (cnd & 2) ? -1. : 1.;
                const double tt[3] = {sg * t[0], sg * t[1], sg * t[2]};
                double q = 0.;
                for (int k = 0; k < 5; ++k) q += epi_score(R, tt, w.f1[k], w.f2[k]);
                if (pass == 0) {
                    if (q < bq) bq = q;
                } else if (q <= bq + 1e-9) {
                    const double tr = R[0] + R[4] + R[8];
                    if (tr > btr) {
                        btr = tr;
                        have = true;
#pragma unroll
                        for (int e = 0; e < 9; ++e) Rout[e] = R[e];
#pragma unroll
                        for (int e = 0; e < 3; ++e) tout[e] = tt[e];
                    }
                }
            }
        }
    return have;
}

// the reference's float roundings of computeSampsonDistance(F, curpt, kfpt) (src/multi_view_geometry.cpp:798-813)
HD inline float epi_sampson(const double F[9], float ucx, float ucy, float ukx, float uky)
{
    const double l[3] = {(double)ucx, (double)ucy, 1.}, r[3] = {(double)ukx, (double)uky, 1.};
    double rF[3], Fl[3];
    for (int j = 0; j < 3; ++j) rF[j] = r[0] * F[j] + r[1] * F[3 + j] + r[2] * F[6 + j];
    for (int i = 0; i < 3; ++i) Fl[i] = F[3 * i] * l[0] + F[3 * i + 1] * l[1] + F[3 * i + 2] * l[2];
    float num = (float)(rF[0] * l[0] + rF[1] * l[1] + rF[2] * l[2]);
    num *= num;
    const float x1 = (float)rF[0], x2 = (float)Fl[0], y1 = (float)rF[1], y2 = (float)Fl[1];
    const float den = x1 * x1 + y1 * y1 + x2 * x2 + y2 * y2;
    return sqrtf(num / den);
}

// F = K^-T [t]x R K^-1 (computeFundamentalMat12(I, T(R, t), K), :824-838)
HD inline void epi_fundamental(const double R[9], const double t[3], const double K[4], double F[9])
{
    const double ki[9] = {1. / K[0], 0., -K[2] / K[0], 0., 1. / K[1], -K[3] / K[1], 0., 0., 1.};
    double E[9], T1[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
            E[3 * i + j] = t[i1] * R[3 * i2 + j] - t[i2] * R[3 * i1 + j];
        }
    for (int i = 0; i < 3; ++i)   // K^-T E
        for (int j = 0; j < 3; ++j) T1[3 * i + j] = ki[i] * E[j] + ki[3 + i] * E[3 + j] + ki[6 + i] * E[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = T1[3 * i] * ki[j] + T1[3 * i + 1] * ki[3 + j] + T1[3 * i + 2] * ki[6 + j];
}

HD inline double epi_threshold(double fx, double fy, float errth)
{   // :654-658: float focal, float quotient; the unqualified atan / cos resolve to the double C functions
    float focal = (float)fx + (float)fy;
    focal /= 2.;
    const float q = errth / focal;
    return 2.0 * (1.0 - cos(atan((double)q)));
}

struct epi_args {
    int nmaxiter;
    float errth;
    const int32_t *off, *goff;
    const double *bv_kf, *bv_cur;
    const float *g_kf, *g_cur;
    const double *K;
    const uint64_t *seed;
    double *R, *t;
    uint8_t *outlier, *gate_bad;
    int32_t *status, *info;
};

struct epi_shared {
    double model[EPI_ROUND][12];
    double best[12];
    double k;
    int ok[EPI_ROUND], cnt[EPI_ROUND];
    int iterations, skipped, best_cnt, best_d, done;
};

__device__ inline void load_pair(const epi_args &A, int g, double f1[3], double f2[3])
{
    for (int k = 0; k < 3; ++k) { f1[k] = A.bv_kf[3 * (size_t)g + k]; f2[k] = A.bv_cur[3 * (size_t)g + k]; }
}

__global__ __launch_bounds__(EPI_THREADS) void epipolar_kernel(epi_args A)
{
    __shared__ epi_shared S;
    __shared__ epi_ws W[EPI_ROUND];   // the solving lanes' workspaces
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o0 = A.off[b], n = A.off[b + 1] - o0;
    const int g0 = A.goff ? A.goff[b] : 0, ng = A.goff ? A.goff[b + 1] - g0 : 0;
    const double K[4] = {A.K[4 * b], A.K[4 * b + 1], A.K[4 * b + 2], A.K[4 * b + 3]};
    const double th = epi_threshold(K[0], K[1], A.errth);
    const uint64_t seed = A.seed[b];
    const int max_iter = A.nmaxiter, max_skip = 10 * A.nmaxiter;
    if (tid == 0) {
        S.iterations = 0; S.skipped = 0; S.best_cnt = -INT_MAX; S.best_d = -1; S.k = 1.0;
        S.done = n < 8 || max_skip <= 0;   // the loop's first test: 0 < k = 1 && 0 < 10 max_iter
    }
    __syncthreads();
    for (int d0 = 0; !S.done; d0 += EPI_ROUND) {
        if (tid < EPI_ROUND) {
            epi_ws &w = W[tid];
            sac_draw<5>(seed, d0 + tid, n, w.idx);
            for (int s = 0; s < 5; ++s) load_pair(A, o0 + w.idx[s], w.f1[s], w.f2[s]);
            S.ok[tid] = epi_model(w, &S.model[tid][0], &S.model[tid][9]);
            S.cnt[tid] = 0;
        }
        __syncthreads();
        for (int r = 0; r < EPI_ROUND; ++r) {
            if (!S.ok[r]) continue;
            double R[9], t[3];
            for (int e = 0; e < 9; ++e) R[e] = S.model[r][e];
            for (int e = 0; e < 3; ++e) t[e] = S.model[r][9 + e];
            int c = 0;
            for (int i = tid; i < n; i += EPI_THREADS) {
                double f1[3], f2[3];
                load_pair(A, o0 + i, f1, f2);
                c += epi_score(R, t, f1, f2) < th;
            }
            if (c) atomicAdd(&S.cnt[r], c);
        }
        __syncthreads();
        if (tid == 0) {   // OpenGV's loop over the round's draws, in draw order
            for (int r = 0; r < EPI_ROUND && !S.done; ++r) {
                if (!(S.iterations < S.k && S.skipped < max_skip)) { S.done = 1; break; }
                if (!S.ok[r]) { ++S.skipped; continue; }
                if (S.cnt[r] > S.best_cnt) {
                    S.best_cnt = S.cnt[r];
                    S.best_d = d0 + r;
                    for (int e = 0; e < 12; ++e) S.best[e] = S.model[r][e];
                    S.k = sac_ransac_k(S.best_cnt, n, 5.0);
                }
                ++S.iterations;
                if (S.iterations > max_iter) S.done = 1;
            }
            if (!(S.iterations < S.k && S.skipped < max_skip)) S.done = 1;
        }
        __syncthreads();
    }
    // status: 0 = the reference's false, 1 = too many outliers (nothing removed), 2 = applied
    const int ninl = S.best_d >= 0 ? S.best_cnt : 0;
    const int status = (S.best_d < 0 || ninl < 10) ? 0 : (2 * (n - ninl) > n ? 1 : 2);
    double R[9], t[3];
    for (int e = 0; e < 9; ++e) R[e] = S.best[e];
    for (int e = 0; e < 3; ++e) t[e] = S.best[9 + e];
    for (int i = tid; i < n; i += EPI_THREADS) {
        uint8_t o = 0;
        if (status >= 1) {
            double f1[3], f2[3];
            load_pair(A, o0 + i, f1, f2);
            o = !(epi_score(R, t, f1, f2) < th);
        }
        A.outlier[o0 + i] = o;
    }
    if (ng > 0) {
        double F[9];
        if (status == 2) epi_fundamental(R, t, K, F);
        for (int i = tid; i < ng; i += EPI_THREADS) {
            uint8_t bad = 0;
            if (status == 2) {
                const size_t g = (size_t)(g0 + i);
                bad = epi_sampson(F, A.g_cur[2 * g], A.g_cur[2 * g + 1], A.g_kf[2 * g], A.g_kf[2 * g + 1]) > A.errth;
            }
            A.gate_bad[g0 + i] = bad;
        }
    }
    if (tid == 0) {
        A.status[b] = status;
        if (status >= 1) {
            for (int e = 0; e < 9; ++e) A.R[9 * b + e] = R[e];
            for (int e = 0; e < 3; ++e) A.t[3 * b + e] = t[e];
        }
        if (A.info) {
            A.info[4 * b] = S.iterations; A.info[4 * b + 1] = S.skipped; A.info[4 * b + 2] = S.best_d;
            A.info[4 * b + 3] = S.best_d >= 0 ? S.best_cnt : 0;
        }
    }
}

__global__ __launch_bounds__(FIVEPT_THREADS) void fivept_dbg_kernel(int n, const double *bv1, const double *bv2, double *E,
                                                                  int32_t *nsol)
{
    __shared__ epi_ws W[FIVEPT_THREADS];
    const int i = blockIdx.x * FIVEPT_THREADS + threadIdx.x;
    if (i >= n) return;
    epi_ws &w = W[threadIdx.x];
    for (int s = 0; s < 5; ++s)
        for (int k = 0; k < 3; ++k) { w.f1[s][k] = bv1[15 * (size_t)i + 3 * s + k]; w.f2[s][k] = bv2[15 * (size_t)i + 3 * s + k]; }
    const int ns = fivept_nister(w);
    for (int s = 0; s < 10; ++s)
        for (int e = 0; e < 9; ++e) E[90 * (size_t)i + 9 * s + e] = s < ns ? w.Es[s][e] : 0.;
    nsol[i] = ns;
}

}  // namespace

extern "C" ov2_status ov2_epipolar_filter_batch_dev(ov2_ctx *c, int B, const int32_t *d_off, const double *d_bv_kf,
                                                    const double *d_bv_cur, const int32_t *d_gate_off,
                                                    const float *d_gate_unpx_kf, const float *d_gate_unpx_cur,
                                                    const double *d_K, int nmaxiter, float errth, const uint64_t *d_seed,
                                                    double *d_R, double *d_t, uint8_t *d_outlier, uint8_t *d_gate_bad,
                                                    int32_t *d_status, int32_t *d_info)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || (B && (!d_off || !d_K || !d_seed || !d_R || !d_t || !d_status || !d_bv_kf || !d_bv_cur || !d_outlier)))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_epipolar_filter_batch_dev: null argument");
    if (d_gate_off && (!d_gate_unpx_kf || !d_gate_unpx_cur || !d_gate_bad))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_epipolar_filter_batch_dev: null gate arrays");
    if (nmaxiter < 0 || nmaxiter > OV2_EPI_MAX_ITER)   // 11 nmaxiter + 1 draws and 10 nmaxiter skips must fit an int
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_epipolar_filter_batch: nmaxiter %d outside [0, %d]", nmaxiter, OV2_EPI_MAX_ITER);
    if (B == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    epi_args A;
    A.nmaxiter = nmaxiter; A.errth = errth; A.off = d_off; A.goff = d_gate_off; A.bv_kf = d_bv_kf; A.bv_cur = d_bv_cur;
    A.g_kf = d_gate_unpx_kf; A.g_cur = d_gate_unpx_cur; A.K = d_K; A.seed = d_seed; A.R = d_R; A.t = d_t;
    A.outlier = d_outlier; A.gate_bad = d_gate_bad; A.status = d_status; A.info = d_info;
    OV2_LAUNCH(c, K_EPI, epipolar_kernel, dim3(B), dim3(EPI_THREADS), 0, c->stream, A);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}

extern "C" ov2_status ov2_epipolar_filter_batch(ov2_ctx *c, int B, const int *n_pairs, const double *bv_kf,
                                                const double *bv_cur, const int *n_gate, const float *gate_unpx_kf,
                                                const float *gate_unpx_cur, const double *K, int nmaxiter, float errth,
                                                const uint64_t *seed, double *R_kfc, double *t_kfc, uint8_t *outlier,
                                                uint8_t *gate_bad, int *status, int *info)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0 || (B && (!n_pairs || !K || !seed || !R_kfc || !t_kfc || !status)))
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_epipolar_filter_batch: null argument");
    if (nmaxiter < 0 || nmaxiter > OV2_EPI_MAX_ITER)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_epipolar_filter_batch: nmaxiter %d outside [0, %d]", nmaxiter, OV2_EPI_MAX_ITER);
    if (B == 0) return OV2_OK;
    size_t n = 0, ng = 0;
    for (int b = 0; b < B; ++b) {
        if (n_pairs[b] < 0 || (n_gate && n_gate[b] < 0)) return ov2_set_err(c, OV2_ERR_INVALID, "negative count");
        n += (size_t)n_pairs[b];
        ng += n_gate ? (size_t)n_gate[b] : 0;
    }
    if (n && (!bv_kf || !bv_cur || !outlier)) return ov2_set_err(c, OV2_ERR_INVALID, "null pair arrays");
    if (ng && (!gate_unpx_kf || !gate_unpx_cur || !gate_bad)) return ov2_set_err(c, OV2_ERR_INVALID, "null gate arrays");
    OV2_HIP(c, hipSetDevice(c->device));
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // staging block: [off | goff | K | seed | bv_kf | bv_cur | gkf | gcur || R | t | status | info | outlier | gate_bad]
    const size_t o_off = 0, o_goff = up(sizeof(int) * (B + 1)), o_K = o_goff + up(sizeof(int) * (B + 1));
    const size_t o_seed = o_K + up(sizeof(double) * 4 * B), o_b1 = o_seed + up(sizeof(uint64_t) * B);
    const size_t o_b2 = o_b1 + up(sizeof(double) * 3 * n), o_g1 = o_b2 + up(sizeof(double) * 3 * n);
    const size_t o_g2 = o_g1 + up(sizeof(float) * 2 * ng), o_R = o_g2 + up(sizeof(float) * 2 * ng);
    const size_t o_t = o_R + up(sizeof(double) * 9 * B), o_st = o_t + up(sizeof(double) * 3 * B);
    const size_t o_in = o_st + up(sizeof(int) * B), o_out = o_in + up(sizeof(int) * 4 * B), o_gb = o_out + up(n);
    const size_t total = o_gb + up(ng);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    {
        int *off = (int *)(hp + o_off), *goff = (int *)(hp + o_goff);
        off[0] = goff[0] = 0;
        for (int b = 0; b < B; ++b) { off[b + 1] = off[b] + n_pairs[b]; goff[b + 1] = goff[b] + (n_gate ? n_gate[b] : 0); }
    }
    memcpy(hp + o_K, K, sizeof(double) * 4 * B);
    memcpy(hp + o_seed, seed, sizeof(uint64_t) * B);
    if (n) { memcpy(hp + o_b1, bv_kf, sizeof(double) * 3 * n); memcpy(hp + o_b2, bv_cur, sizeof(double) * 3 * n); }
    if (ng) { memcpy(hp + o_g1, gate_unpx_kf, sizeof(float) * 2 * ng); memcpy(hp + o_g2, gate_unpx_cur, sizeof(float) * 2 * ng); }
    memcpy(hp + o_R, R_kfc, sizeof(double) * 9 * B);   // untouched where the status is 0
    memcpy(hp + o_t, t_kfc, sizeof(double) * 3 * B);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_st, hipMemcpyHostToDevice, st));
    s = ov2_epipolar_filter_batch_dev(c, B, (const int32_t *)(dp + o_off), (const double *)(dp + o_b1),
                                      (const double *)(dp + o_b2), (const int32_t *)(dp + o_goff), (const float *)(dp + o_g1),
                                      (const float *)(dp + o_g2), (const double *)(dp + o_K), nmaxiter, errth,
                                      (const uint64_t *)(dp + o_seed), (double *)(dp + o_R), (double *)(dp + o_t),
                                      (uint8_t *)(dp + o_out), (uint8_t *)(dp + o_gb), (int32_t *)(dp + o_st),
                                      (int32_t *)(dp + o_in));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_R, dp + o_R, total - o_R, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(R_kfc, hp + o_R, sizeof(double) * 9 * B);
    memcpy(t_kfc, hp + o_t, sizeof(double) * 3 * B);
    memcpy(status, hp + o_st, sizeof(int) * B);
    if (info) memcpy(info, hp + o_in, sizeof(int) * 4 * B);
    if (n) memcpy(outlier, hp + o_out, n);
    if (ng) memcpy(gate_bad, hp + o_gb, ng);
    return OV2_OK;
}

extern "C" ov2_status ov2_dbg_fivept(ov2_ctx *c, int n, const double *bv1, const double *bv2, double *E, int *nsol)
{
    if (!c) return OV2_ERR_INVALID;
    if (n < 0 || (n && (!bv1 || !bv2 || !E || !nsol))) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_dbg_fivept: null argument");
    if (n == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_b1 = 0, o_b2 = up(sizeof(double) * 15 * n), o_E = o_b2 + up(sizeof(double) * 15 * n);
    const size_t o_ns = o_E + up(sizeof(double) * 90 * n), total = o_ns + up(sizeof(int) * n);
    char *hp = nullptr, *dp = nullptr;
    ov2_status s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    memcpy(hp + o_b1, bv1, sizeof(double) * 15 * n);
    memcpy(hp + o_b2, bv2, sizeof(double) * 15 * n);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_E, hipMemcpyHostToDevice, st));
    OV2_LAUNCH(c, K_FIVEPT, fivept_dbg_kernel, dim3((n + FIVEPT_THREADS - 1) / FIVEPT_THREADS), dim3(FIVEPT_THREADS), 0, st, n, (const double *)(dp + o_b1),
               (const double *)(dp + o_b2), (double *)(dp + o_E), (int32_t *)(dp + o_ns));
    OV2_HIP(c, hipGetLastError());
    OV2_HIP(c, hipMemcpyAsync(hp + o_E, dp + o_E, total - o_E, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(E, hp + o_E, sizeof(double) * 90 * n);
    memcpy(nsol, hp + o_ns, sizeof(int) * n);
    return OV2_OK;
}
