// orbm_sim3_math.h -- g2o's Sim3 (Thirdparty/g2o/g2o/types/sim3.h) as the two Sim3 optimisers share it (orbm_sim3opt.hip:
// OptimizeSim3, orbm_essential_graph.hip: OptimizeEssentialGraph): the constructor from R, t, s, the exponential map, the product
// and the inverse, in the reference's operation order.  Everything here is inline: two translation units include it.
#pragma once
#include "orbm_g2o_math.h"

namespace orbm_detail {

struct Sim3 { double q[4], t[3], s; };  // q = x y z w

// ------------------------------------------------------------------ sim3.h

__host__ __device__ inline void sim3_from_rts(const float *R, const float *t, float s, Sim3 &o)   // :64-67 from the float inputs
{
    double Rd[9];
    for (int k = 0; k < 9; ++k) Rd[k] = R[k];
    quat_from_matrix(Rd, o.q);
    for (int k = 0; k < 3; ++k) o.t[k] = t[k];
    o.s = s;
}

__device__ inline void sim3_exp(const double u[7], Sim3 &o)   // Sim3(const Vector7d&), :70-142
{
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double Om[9] = {0., -w2, w1, w2, 0., -w0, -w1, w0, 0.};
    const double s = exp(sigma);
    double O2[9], R[9], A, B, C;
    ORBM_UNROLL for (int i = 0; i < 3; ++i)
        ORBM_UNROLL for (int j = 0; j < 3; ++j) O2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    const double eps = 0.00001;
    const bool small_theta = theta < eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    if (small_theta) {      // the first-order rotation: not orthogonal, and its quaternion is taken unnormalised
        ORBM_UNROLL for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
    } else {
        const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
        ORBM_UNROLL for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + ra * Om[k] + rb * O2[k];
    }
    quat_from_matrix(R, o.q);
    double W[9];
    ORBM_UNROLL for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + B * O2[k] + C * ((k % 4 == 0) ? 1.0 : 0.0);
    ORBM_UNROLL for (int i = 0; i < 3; ++i) o.t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o.s = s;
}

__device__ __forceinline__ void sim3_mul(const Sim3 &A, const Sim3 &B, Sim3 &O)   // :266-272
{
    Sim3 r;
    double rt[3];
    const double *a = A.q, *b = B.q;
    r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    q_rotate(A.q, B.t, rt);
    ORBM_UNROLL for (int k = 0; k < 3; ++k) r.t[k] = A.s * rt[k] + A.t[k];
    r.s = A.s * B.s;
    O = r;
}

__device__ __forceinline__ void sim3_inverse(const Sim3 &A, Sim3 &O)   // :233-236
{
    Sim3 r;
    const double f = -1. / A.s;
    const double v[3] = {f * A.t[0], f * A.t[1], f * A.t[2]};
    r.q[0] = -A.q[0]; r.q[1] = -A.q[1]; r.q[2] = -A.q[2]; r.q[3] = A.q[3];
    q_rotate(r.q, v, r.t);
    r.s = 1. / A.s;
    O = r;
}

} // namespace orbm_detail
