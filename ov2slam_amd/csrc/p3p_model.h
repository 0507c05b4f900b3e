// p3p_model.h -- the model of the P3P sample-consensus stage (p3p.hip), host + device so that a CPU build can be
// compared with the kernels: Kneip's P3P (Kneip, Scaramuzza, Siegwart, CVPR 2011; OpenGV's KNEIP algorithm of
// AbsolutePoseSacProblem), the 4th-point pick, the distance 1 - f . p / |p| and the threshold.
//   * the quartic in cos(theta) of the paper, its real roots in [-1, 1] by the bounded bracketing of sac_common.h (OpenGV
//     takes the real parts of all four complex roots; a draw without a real solution is "no model" here);
//   * each root gives the camera centre C, so the three depths s_i = |X_i - C|.  The depths are polished by Newton on
//     the three distance constraints |s_i f_i - s_j f_j|^2 = |X_i - X_j|^2 (Kneip's chain loses digits on some samples),
//     and [R | t] is rebuilt from the two congruent triangles through orthonormal frames, so R is a rotation to
//     rounding whatever the conditioning.  A candidate that does not map the three points onto their bearings with
//     positive depth to 1e-10, or that repeats an earlier one, is dropped.
#pragma once
#include "sac_common.h"

HD inline double p3p_sqrt(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

struct p3p_ws { double p[5], q[5], cp[4], nr[4]; };   // per-lane workspace of the root finder (LDS in the kernels)

HD inline void p3p_cross(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
HD inline double p3p_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
HD inline bool p3p_unit(double *a)
{
    const double n = p3p_sqrt(p3p_dot(a, a));
    a[0] /= n; a[1] /= n; a[2] /= n;
    return n > 0. && n < INFINITY;
}
// orthonormal frame of the triangle (a, b, c): e1 along b - a, e3 the normal, e2 = e3 x e1
HD inline bool p3p_frame(const double *a, const double *b, const double *c, double e[3][3])
{
    double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    for (int k = 0; k < 3; ++k) e[0][k] = u[k];
    bool ok = p3p_unit(e[0]);
    p3p_cross(u, v, e[2]);
    ok = p3p_unit(e[2]) && ok;
    p3p_cross(e[2], e[0], e[1]);
    return ok;
}

// distance of a correspondence (bearing f, world point X) to the model [R | t] (camera to world, R row-major):
// p = R^T (X - t), 1 - f . p / |p|.  Unclamped: the 4th-point score of the model pick.
HD inline double p3p_score(const double R[9], const double t[3], const double *f, const double *X)
{
    const double v0 = X[0] - t[0], v1 = X[1] - t[1], v2 = X[2] - t[2];
    const double p0 = R[0] * v0 + R[3] * v1 + R[6] * v2, p1 = R[1] * v0 + R[4] * v1 + R[7] * v2;
    const double p2 = R[2] * v0 + R[5] * v1 + R[8] * v2;
    const double n = p3p_sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    return 1.0 - (f[0] * (p0 / n) + f[1] * (p1 / n) + f[2] * (p2 / n));
}
// the distance the loops sort and classify: clamped below at 0, a non-finite one counts as +infinity
HD inline double p3p_dist(const double R[9], const double t[3], const double *f, const double *X)
{
    const double d = p3p_score(R, t, f, X);
    if (!(fabs(d) < INFINITY)) return INFINITY;
    return d < 0. ? 0. : d;
}

HD inline double p3p_threshold(double fx, double fy, float errth)
{   // src/multi_view_geometry.cpp:298-302: float focal, float quotient; atan / cos are the double C functions
    float focal = (float)fx + (float)fy;
    focal /= 2.;
    const float q = errth / focal;
    return 1.0 - cos(atan((double)q));
}

// Kneip's P3P on the bearings f[0..2] and world points X[0..2]; emit(R, t) is called for every solution [R_wc | t_wc]
// (at most 4, in ascending order of the root cos(theta)).  Returns their number.
template <class Emit>
HD inline int p3p_kneip(const double f[3][3], const double X[3][3], p3p_ws &w, Emit &&emit)
{
    double F[3][3], P[3][3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) { F[i][k] = f[i][k]; P[i][k] = X[i][k]; }
    {
        const double a[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        const double b[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        double c[3];
        p3p_cross(a, b, c);
        if (!(p3p_dot(c, c) > 0.)) return 0;   // collinear (or non-finite) world points
    }
    // intermediate camera frame tau = (f1, f3' , f1 x f2); the third bearing must have a negative z there
    double T[3][3], f3[3];
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < 3; ++k) T[0][k] = F[0][k];
        p3p_cross(F[0], F[1], T[2]);
        if (!p3p_unit(T[2])) return 0;
        p3p_cross(T[2], T[0], T[1]);
        for (int i = 0; i < 3; ++i) f3[i] = p3p_dot(T[i], F[2]);
        if (pass == 1 || !(f3[2] > 0.)) break;
        for (int k = 0; k < 3; ++k) {
            double s = F[0][k]; F[0][k] = F[1][k]; F[1][k] = s;
            s = P[0][k]; P[0][k] = P[1][k]; P[1][k] = s;
        }
    }
    // intermediate world frame eta: the world triangle's orthonormal frame, also what the candidates' [R | t] are built on
    double N[3][3];
    if (!p3p_frame(P[0], P[1], P[2], N)) return 0;
    const double d3[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const double d2[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const double p_1 = p3p_dot(N[0], d3), p_2 = p3p_dot(N[1], d3);
    const double d_12 = p3p_sqrt(p3p_dot(d2, d2));
    const double f_1 = f3[0] / f3[2], f_2 = f3[1] / f3[2];
    const double cos_beta = p3p_dot(F[0], F[1]);
    double b = 1. / (1. - cos_beta * cos_beta) - 1.;
    b = cos_beta < 0. ? -p3p_sqrt(b) : p3p_sqrt(b);
    const double f_1_pw2 = f_1 * f_1, f_2_pw2 = f_2 * f_2, p_1_pw2 = p_1 * p_1, p_1_pw3 = p_1_pw2 * p_1, p_1_pw4 = p_1_pw3 * p_1;
    const double p_2_pw2 = p_2 * p_2, p_2_pw3 = p_2_pw2 * p_2, p_2_pw4 = p_2_pw3 * p_2, d_12_pw2 = d_12 * d_12, b_pw2 = b * b;
    w.p[4] = -f_2_pw2 * p_2_pw4 - p_2_pw4 * f_1_pw2 - p_2_pw4;
    w.p[3] = 2. * p_2_pw3 * d_12 * b + 2. * f_2_pw2 * p_2_pw3 * d_12 * b - 2. * f_2 * p_2_pw3 * f_1 * d_12;
    w.p[2] = -f_2_pw2 * p_2_pw2 * p_1_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2 - f_2_pw2 * p_2_pw2 * d_12_pw2 + f_2_pw2 * p_2_pw4
           + p_2_pw4 * f_1_pw2 + 2. * p_1 * p_2_pw2 * d_12 + 2. * f_1 * f_2 * p_1 * p_2_pw2 * d_12 * b - p_2_pw2 * p_1_pw2 * f_1_pw2
           + 2. * p_1 * p_2_pw2 * f_2_pw2 * d_12 - p_2_pw2 * d_12_pw2 * b_pw2 - 2. * p_1_pw2 * p_2_pw2;
    w.p[1] = 2. * p_1_pw2 * p_2 * d_12 * b + 2. * f_2 * p_2_pw3 * f_1 * d_12 - 2. * f_2_pw2 * p_2_pw3 * d_12 * b - 2. * p_1 * p_2 * d_12_pw2 * b;
    w.p[0] = -2. * f_2 * p_2_pw2 * f_1 * p_1 * d_12 * b + f_2_pw2 * p_2_pw2 * d_12_pw2 + 2. * p_1_pw3 * d_12 - p_1_pw2 * d_12_pw2
           + f_2_pw2 * p_2_pw2 * p_1_pw2 - p_1_pw4 - 2. * f_2_pw2 * p_2_pw2 * p_1 * d_12 + p_2_pw2 * f_1_pw2 * p_1_pw2
           + f_2_pw2 * p_2_pw2 * d_12_pw2 * b_pw2;
    for (int i = 0; i < 5; ++i)
        if (!(fabs(w.p[i]) < INFINITY)) return 0;
    int deg = 4;
    while (deg > 0 && w.p[deg] == 0.) --deg;
    if (deg == 0) return 0;
    const int nroots = sac_real_roots_in(w.p, deg, -1., 1., w.q, w.cp, w.nr);   // cos(theta): nothing outside [-1, 1] is admissible

    const double c01 = p3p_dot(F[0], F[1]), c02 = p3p_dot(F[0], F[2]), c12 = p3p_dot(F[1], F[2]);
    double e01 = 0., e02 = 0., e12 = 0.;
    for (int k = 0; k < 3; ++k) {
        e01 += (P[0][k] - P[1][k]) * (P[0][k] - P[1][k]);
        e02 += (P[0][k] - P[2][k]) * (P[0][k] - P[2][k]);
        e12 += (P[1][k] - P[2][k]) * (P[1][k] - P[2][k]);
    }
    double prev[4][3];
    int ns = 0;
    for (int r = 0; r < nroots; ++r) {
        const double cos_theta = w.cp[r];
        const double st2 = 1. - cos_theta * cos_theta;
        if (!(st2 >= 0.)) continue;
        const double sin_theta = p3p_sqrt(st2);
        const double cot_alpha = (-f_1 * p_1 / f_2 - cos_theta * p_2 + d_12 * b) / (-f_1 * cos_theta * p_2 / f_2 + p_1 - d_12);
        const double sin_alpha = p3p_sqrt(1. / (cot_alpha * cot_alpha + 1.));
        double cos_alpha = p3p_sqrt(1. - sin_alpha * sin_alpha);
        if (cot_alpha < 0.) cos_alpha = -cos_alpha;
        const double m = d_12 * (sin_alpha * b + cos_alpha);
        const double Ce[3] = {cos_alpha * m, cos_theta * sin_alpha * m, sin_theta * sin_alpha * m};
        double s[3];
        for (int i = 0; i < 3; ++i) {   // depth of point i: |P_i - C|, C = P_0 + N^T Ce
            double dd = 0.;
            for (int k = 0; k < 3; ++k) {
                const double ck = P[0][k] + (N[0][k] * Ce[0] + N[1][k] * Ce[1] + N[2][k] * Ce[2]);
                dd += (P[i][k] - ck) * (P[i][k] - ck);
            }
            s[i] = p3p_sqrt(dd);
        }
        // Newton on g_ij = s_i^2 + s_j^2 - 2 s_i s_j c_ij - e_ij (at most 4 steps; a step that does not lower |g| is undone)
        double gprev = INFINITY, sv[3] = {s[0], s[1], s[2]};
#pragma unroll 1
        for (int it = 0; it < 5; ++it) {
            const double g0 = s[0] * s[0] + s[1] * s[1] - 2. * s[0] * s[1] * c01 - e01;
            const double g1 = s[0] * s[0] + s[2] * s[2] - 2. * s[0] * s[2] * c02 - e02;
            const double g2 = s[1] * s[1] + s[2] * s[2] - 2. * s[1] * s[2] * c12 - e12;
            const double gn = fabs(g0) + fabs(g1) + fabs(g2);
            if (!(gn < gprev)) { s[0] = sv[0]; s[1] = sv[1]; s[2] = sv[2]; break; }
            gprev = gn;
            sv[0] = s[0]; sv[1] = s[1]; sv[2] = s[2];
            if (gn == 0. || it == 4) break;
            const double a00 = 2. * (s[0] - s[1] * c01), a01 = 2. * (s[1] - s[0] * c01);
            const double a10 = 2. * (s[0] - s[2] * c02), a12 = 2. * (s[2] - s[0] * c02);
            const double a21 = 2. * (s[1] - s[2] * c12), a22 = 2. * (s[2] - s[1] * c12);
            // [a00 a01 0; a10 0 a12; 0 a21 a22] ds = -g
            const double det = -a00 * a12 * a21 - a01 * a10 * a22;
            const double x0 = (-g0 * (-a12 * a21) - a01 * (-g1 * a22 + a12 * g2)) / det;
            const double x1 = (a00 * (-g1 * a22 + a12 * g2) + g0 * a10 * a22) / det;
            const double x2 = (a00 * (g1 * a21) - a01 * a10 * (-g2) - g0 * a10 * a21) / det;
            s[0] += x0; s[1] += x1; s[2] += x2;
        }
        if (!(s[0] > 0. && s[1] > 0. && s[2] > 0.)) continue;
        bool dup = false;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < ns)
                dup = dup || (fabs(prev[q][0] - s[0]) <= 1e-9 * s[0] && fabs(prev[q][1] - s[1]) <= 1e-9 * s[1] &&
                              fabs(prev[q][2] - s[2]) <= 1e-9 * s[2]);
        if (dup) continue;
        // [R | t]: the camera triangle s_i f_i onto the world triangle
        double A[3][3], E[3][3];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) A[i][k] = s[i] * F[i][k];
        if (!p3p_frame(A[0], A[1], A[2], E)) continue;
        double R[9], t[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = N[0][i] * E[0][j] + N[1][i] * E[1][j] + N[2][i] * E[2][j];
        for (int i = 0; i < 3; ++i) {
            const double ma[3] = {(A[0][0] + A[1][0] + A[2][0]) / 3., (A[0][1] + A[1][1] + A[2][1]) / 3., (A[0][2] + A[1][2] + A[2][2]) / 3.};
            t[i] = (P[0][i] + P[1][i] + P[2][i]) / 3. - (R[3 * i] * ma[0] + R[3 * i + 1] * ma[1] + R[3 * i + 2] * ma[2]);
        }
        bool good = true;
        for (int i = 0; i < 3; ++i) {
            const double v0 = P[i][0] - t[0], v1 = P[i][1] - t[1], v2 = P[i][2] - t[2];
            const double q0 = R[0] * v0 + R[3] * v1 + R[6] * v2, q1 = R[1] * v0 + R[4] * v1 + R[7] * v2, q2 = R[2] * v0 + R[5] * v1 + R[8] * v2;
            const double n = p3p_sqrt(q0 * q0 + q1 * q1 + q2 * q2);
            const double err = fmax(fabs(q0 / n - F[i][0]), fmax(fabs(q1 / n - F[i][1]), fabs(q2 / n - F[i][2])));
            good = good && err < 1e-10;
        }
        if (!good) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q == ns) { prev[q][0] = s[0]; prev[q][1] = s[1]; prev[q][2] = s[2]; }
        emit(R, t);
        ++ns;
    }
    return ns;
}

// OpenGV AbsolutePoseSacProblem::computeModelCoefficients (KNEIP): P3P on the first three correspondences, the fourth
// picks the solution with the lowest score.  model = R (9) then t (3).  false = no model for this draw.
HD inline bool p3p_model(const double f[4][3], const double X[4][3], p3p_ws &w, double model[12])
{
    double best = INFINITY;
    bool have = false;
    p3p_kneip(f, X, w, [&](const double *R, const double *t) {
        const double sc = p3p_score(R, t, f[3], X[3]);
        if (sc < best) {
            best = sc;
            have = true;
            for (int e = 0; e < 9; ++e) model[e] = R[e];
            for (int e = 0; e < 3; ++e) model[9 + e] = t[e];
        }
    });
    return have;
}
