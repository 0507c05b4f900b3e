// tri_pair.h -- the per-pair arithmetic of the mapper's two triangulation stages as device functions, shared by
// tri_kernel (tri.hip: pairs handed in as flat arrays) and the temporal stage on the map mirror (map.hip: pairs read off
// the observation table).  Arithmetic and operation order are those of oracle/ov2_oracle_tri.c (f64, contraction off);
// every R[9] / X[3] is indexed statically so that nothing spills to private memory.  The pose arithmetic (tri_quat_R,
// tri_apply) is in ov2_se3.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ov2slam_hip.h"
#include "ov2_se3.h"

namespace ov2tri {

// CameraCalibration::projectCamToImage (src/camera_calibration.cpp:243-252)
__device__ __forceinline__ void project(const double K[4], const double p[3], float &u, float &v)
{
    const double invz = 1. / p[2];
    const double x = p[0] * invz, y = p[1] * invz;
    u = (float)(K[0] * x + K[2]);
    v = (float)(K[1] * y + K[3]);
}

// cv::norm(Point2f - Point2f): float differences, square root in double
__device__ __forceinline__ double norm2f(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return __dsqrt_rn((double)dx * dx + (double)dy * dy);
}

// R_ab * f2: the bearing of view b in the frame of view a
__device__ __forceinline__ void rotate(const double R[9], const double f2[3], double f2u[3])
{
    f2u[0] = R[0] * f2[0] + R[1] * f2[1] + R[2] * f2[2];
    f2u[1] = R[3] * f2[0] + R[4] * f2[1] + R[5] * f2[2];
    f2u[2] = R[6] * f2[0] + R[7] * f2[1] + R[8] * f2[2];
}

// rotation-compensated parallax (src/mapper.cpp:298-299): |unpx_a - proj(R_ab * bv_b)|
__device__ __forceinline__ double parallax_px(const double Kb[4], const double f2u[3], float ua, float va)
{
    float ru, rv;
    project(Kb, f2u, ru, rv);
    return norm2f(ua, va, ru, rv);
}

// OpenGV's mid-point method (triangulation/methods.cpp triangulate2; src/multi_view_geometry.cpp:85-99): point in frame a
__device__ __forceinline__ void midpoint(const double *T, const double f1[3], const double f2u[3], double X[3])
{
    const double a00 = f1[0] * f1[0] + f1[1] * f1[1] + f1[2] * f1[2];
    const double a10 = f1[0] * f2u[0] + f1[1] * f2u[1] + f1[2] * f2u[2];
    const double a01 = -a10;
    const double a11 = -(f2u[0] * f2u[0] + f2u[1] * f2u[1] + f2u[2] * f2u[2]);
    const double b0 = T[0] * f1[0] + T[1] * f1[1] + T[2] * f1[2];
    const double b1 = T[0] * f2u[0] + T[1] * f2u[1] + T[2] * f2u[2];
    const double invdet = 1. / (a00 * a11 - a01 * a10);
    const double l0 = (a11 * invdet) * b0 + (-a01 * invdet) * b1;
    const double l1 = (-a10 * invdet) * b0 + (a00 * invdet) * b1;
    X[0] = (l0 * f1[0] + (T[0] + l1 * f2u[0])) / 2.;
    X[1] = (l0 * f1[1] + (T[1] + l1 * f2u[1])) / 2.;
    X[2] = (l0 * f1[2] + (T[2] + l1 * f2u[2])) / 2.;
}

// the rectified disparity form (src/mapper.cpp:410-422): depth fx * |t| / |disp| kept as the float the reference holds, the
// left pixel back-projected with iK.  false: negative disparity (:413-416), X untouched
__device__ __forceinline__ bool rectified(const double *T, const double Ka[4], float ua, float va, float ub, double X[3])
{
    const float disp = ua - ub;
    if (disp < 0.f) return false;
    const double base = __dsqrt_rn(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
    const float z = (float)(Ka[0] * base / fabs((double)disp));
    X[0] = (double)z * ((double)ua / Ka[0] - Ka[2] / Ka[0]);
    X[1] = (double)z * ((double)va / Ka[1] - Ka[3] / Ka[1]);
    X[2] = (double)z;
    return true;
}

// the mapper's acceptance gates (src/mapper.cpp:307-329, :425-445): depth >= 0.1 in both views, then the float
// reprojection distances against max_err.  T / R: view b in the frame of view a
__device__ __forceinline__ int gates(const double *T, const double R[9], const double X[3], const double Ka[4], const double Kb[4],
                                     float ua, float va, float ub, float vb, float max_err)
{
    const double d[3] = {X[0] - T[0], X[1] - T[1], X[2] - T[2]};
    const double Xb[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                          R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
    if (X[2] < 0.1 || Xb[2] < 0.1) return OV2_TRI_BEHIND;
    float pu, pv, qu, qv;
    project(Ka, X, pu, pv);
    project(Kb, Xb, qu, qv);
    const float ldist = (float)norm2f(pu, pv, ua, va), rdist = (float)norm2f(qu, qv, ub, vb);
    return (ldist > max_err || rdist > max_err) ? OV2_TRI_REPROJ : OV2_TRI_OK;
}

}  // namespace ov2tri
