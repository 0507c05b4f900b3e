// ov2_se3.h -- the SE(3) / quaternion arithmetic of the kernels, written once per formula.  A pose is the 7-vector
// [t, qx qy qz qw] (Sophus).  Operation order is that of the oracle file named at each function (f64, contraction off):
// two spellings of the same formula that round differently are two functions here, never one with reordered terms.
#pragma once
#include <hip/hip_runtime.h>

namespace ov2se3 {

// ---- the solvers' form (oracle/ov2_oracle_ba.c, _pnp.c, _pg.c: Eigen's Quaternion::toRotationMatrix) --------------

// unit quaternion (x, y, z, w) -> R, no normalisation
__host__ __device__ inline void quat_to_R(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// rotation of a pose: its quaternion normalised (Eigen::Map<Quaterniond>::normalized()), then quat_to_R
__host__ __device__ inline void pose_R(const double *p, double R[9])
{
    double q[4] = {p[3], p[4], p[5], p[6]};
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
    quat_to_R(q, R);
}

__host__ __device__ inline void pose_Rt(const double *p, double R[9], double t[3])
{
    pose_R(p, R);
    t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
}

// SE3LeftParameterization::Plus: out = Sophus::SE3::exp(d) * SE3(q, t)   (se3left_parametrization.hpp:41-60)
__device__ inline void se3_plus(const double *x, const double *d, double *out)
{
    const double *u = d, *w = d + 3;
    const double eps = 1e-10;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double theta, imag, real;
    if (th2 < eps * eps) {
        theta = 0.0;
        const double th4 = th2 * th2;
        imag = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4;
        real = 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th4;
    } else {
        theta = sqrt(th2);
        const double half = 0.5 * theta;
        imag = sin(half) / theta;
        real = cos(half);
    }
    // exp's quaternion is unit up to rounding and the oracle does not normalise it: the raw form
    const double a[4] = {imag * w[0], imag * w[1], imag * w[2], real};
    double Ra[9], V[9];
    quat_to_R(a, Ra);
    if (theta < eps) {
        for (int i = 0; i < 9; ++i) V[i] = Ra[i];
    } else {
        const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        double O2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += O[3 * i + k] * O[3 * k + j];
                O2[3 * i + j] = s;
            }
        const double t2 = theta * theta;
        const double c1 = (1.0 - cos(theta)) / t2, c2 = (theta - sin(theta)) / (t2 * theta);
        for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + c1 * O[i] + c2 * O2[i];
    }
    double b[4] = {x[3], x[4], x[5], x[6]};
    const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    b[0] /= nb; b[1] /= nb; b[2] /= nb; b[3] /= nb;
    double q[4];
    q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int r = 0; r < 3; ++r)
        out[r] = (V[3 * r] * u[0] + V[3 * r + 1] * u[1] + V[3 * r + 2] * u[2]) +
                 (Ra[3 * r] * x[0] + Ra[3 * r + 1] * x[1] + Ra[3 * r + 2] * x[2]);
    out[3] = q[0] / nq; out[4] = q[1] / nq; out[5] = q[2] / nq; out[6] = q[3] / nq;
}

// rotation part of se3_plus alone: out = exp(w) * b renormalised, b a unit quaternion (x, y, z, w) taken as it is
__device__ inline void quat_plus_left(const double b[4], const double w[3], double out[4])
{
    const double eps = 1e-10;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double imag, real;
    if (th2 < eps * eps) {
        const double th4 = th2 * th2;
        imag = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4;
        real = 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th4;
    } else {
        const double theta = sqrt(th2);
        const double half = 0.5 * theta;
        imag = sin(half) / theta;
        real = cos(half);
    }
    const double a[4] = {imag * w[0], imag * w[1], imag * w[2], real};
    double q[4];
    q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    out[0] = q[0] / nq; out[1] = q[1] / nq; out[2] = q[2] / nq; out[3] = q[3] / nq;
}

// ---- the host mirror's form (SE3::fromRt of ov2_host.cpp) ---------------------------------------------------------

// rotation matrix -> quaternion (x, y, z, w), in the mirror's branch order
__device__ inline void rot_to_quat(const double R[9], double q[4])
{
    const double t = R[0] + R[4] + R[8];
    if (t > 0) {
        const double s = __dsqrt_rn(t + 1.0) * 2;
        q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = __dsqrt_rn(1.0 + R[0] - R[4] - R[8]) * 2;
        q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = __dsqrt_rn(1.0 + R[4] - R[0] - R[8]) * 2;
        q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s;
    } else {
        const double s = __dsqrt_rn(1.0 + R[8] - R[0] - R[4]) * 2;
        q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s;
    }
}

// ---- the triangulation form (oracle/ov2_oracle_tri.c) -------------------------------------------------------------
// __forceinline__ and static indexing of R[9] / X[3]: nothing spills to private memory in the per-pair kernels.

// rotation of a pose whose quaternion is taken as unit: 1 - 2 (yy + zz), no normalisation
__device__ __forceinline__ void tri_quat_R(const double *T, double R[9])
{
    const double x = T[3], y = T[4], z = T[5], w = T[6];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// T * X (Frame::projCamToWorld for T = Twc): rotate, then add t
__device__ __forceinline__ void tri_apply(const double *T, const double X[3], double out[3])
{
    double R[9];
    tri_quat_R(T, R);
    out[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + T[0];
    out[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + T[1];
    out[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + T[2];
}

}  // namespace ov2se3
