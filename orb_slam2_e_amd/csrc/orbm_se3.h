// orbm_se3.h -- g2o's SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) as the double-precision pose solvers use it (orbm_pose.hip:
// PoseOptimization, orbm_pose_nr.hip: PoseOptimizationNR), in the restatements' operation order: exp, product and map in quaternion
// form with g2o's normalisation, Converter::toSE3Quat.  Eigen's part is orbm_g2o_math.h.  Everything is inline.
#pragma once
#include "orbm_g2o_math.h"

namespace orbm_detail {

struct Se3 { double q[4], t[3]; };

// ------------------------------------------------------------------ se3quat.h, in the restatement's operation order (Eigen: orbm_g2o_math.h)

__device__ __forceinline__ void q_normalize(double q[4])
{
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n > 0.0) {
        const double s = sqrt(n);
        q[0] /= s; q[1] /= s; q[2] /= s; q[3] /= s;
    }
}

__device__ __forceinline__ void normalize_rotation(double q[4])   // SE3Quat::normalizeRotation
{
    if (q[3] < 0) { q[0] *= -1; q[1] *= -1; q[2] *= -1; q[3] *= -1; }
    q_normalize(q);
}

__device__ __forceinline__ void quat_to_matrix(const double q[4], double R[9])   // toRotationMatrix
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

__device__ __forceinline__ void se3_map(const Se3 &T, const double X[3], double o[3])   // SE3Quat::map
{
    q_rotate(T.q, X, o);
    o[0] += T.t[0]; o[1] += T.t[1]; o[2] += T.t[2];
}

__device__ inline void se3_exp(const double u[6], Se3 &T)   // SE3Quat::exp
{
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double Om[9] = {0., -w2, w1, w2, 0., -w0, -w1, w0, 0.};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k]; V[k] = R[k]; }
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / (pow(theta, 3.0));
        for (int k = 0; k < 9; ++k) {
            const double I = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = I + a * Om[k] + b * O2[k];
            V[k] = I + b * Om[k] + c * O2[k];
        }
    }
    quat_from_matrix(R, T.q);
    for (int i = 0; i < 3; ++i) T.t[i] = V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
    normalize_rotation(T.q);
}

__device__ inline void se3_compose(const Se3 &A, const Se3 &B, Se3 &O)   // SE3Quat::operator*
{
    Se3 r = A;
    double rt[3];
    q_rotate(A.q, B.t, rt);
    r.t[0] += rt[0]; r.t[1] += rt[1]; r.t[2] += rt[2];
    const double *a = A.q, *b = B.q;
    r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    normalize_rotation(r.q);
    O = r;
}

__device__ inline void se3_from_cv(const float *T, Se3 &o)   // Converter::toSE3Quat
{
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    quat_from_matrix(R, o.q);
    o.t[0] = T[3]; o.t[1] = T[7]; o.t[2] = T[11];
    normalize_rotation(o.q);
}

} // namespace orbm_detail
