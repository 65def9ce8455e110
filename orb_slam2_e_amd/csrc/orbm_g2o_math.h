// orbm_g2o_math.h -- the slice of Eigen and g2o that the double-precision solvers share (orbm_pose.hip: PoseOptimization,
// orbm_sim3opt.hip: OptimizeSim3, orbm_pose_nr.hip: PoseOptimizationNR, orbm_ba.hip: the bundle adjustments,
// orbm_essential_graph.hip: OptimizeEssentialGraph), in the restatements' operation order (tests/g2o_restated.h): Eigen's
// quaternion constructor and rotation, its fixed 3 x 3 inverse and pivoting LDLT, g2o's Huber kernel and Levenberg step rule
// (orbm_levenberg.h, which comes with this file) and the fixed-order wave and block reductions.  What belongs to one problem
// (Se3 / Sim3, the exp maps, the edges) stays in its file.  Everything here is inline: each of the five solvers' translation units includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "orbm_levenberg.h"

#define ORBM_UNROLL _Pragma("unroll")

namespace orbm_detail {

// ------------------------------------------------------------------ Eigen's quaternion

// the trace <= 0 branch with the largest diagonal entry at I (a compile-time index: R and q stay in registers)
template <int I>
__host__ __device__ __forceinline__ void quat_from_matrix_diag(const double R[9], double q[4])
{
#define M(i, j) R[3 * (i) + (j)]
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(M(I, I) - M(J, J) - M(K, K) + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (M(K, J) - M(J, K)) * t;
    q[J] = (M(J, I) + M(I, J)) * t;
    q[K] = (M(K, I) + M(I, K)) * t;
#undef M
}

// Quaterniond(const Matrix3d&): not normalised.  Host too: orbm_optimize_sim3 forms the result of a problem without a pair with it.
__host__ __device__ inline void quat_from_matrix(const double R[9], double q[4])
{
#define M(i, j) R[3 * (i) + (j)]
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (M(2, 1) - M(1, 2)) * t;
        q[1] = (M(0, 2) - M(2, 0)) * t;
        q[2] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > (i == 1 ? M(1, 1) : M(0, 0))) i = 2;
        if (i == 0) quat_from_matrix_diag<0>(R, q);
        else if (i == 1) quat_from_matrix_diag<1>(R, q);
        else quat_from_matrix_diag<2>(R, q);
    }
#undef M
}

__device__ __forceinline__ void q_rotate(const double q[4], const double v[3], double o[3])   // Quaternion * Vector3d
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    ORBM_UNROLL for (int i = 0; i < 3; ++i) o[i] = v[i] + q[3] * uv[i] + c[i];
}

// ------------------------------------------------------------------ Eigen's fixed-size inverse

// LU/InverseImpl.h, compute_inverse<Matrix3d>: the cofactors, the determinant from the first column, every entry a cofactor times
// 1 / det.  A singular block gives non-finite entries, as there.
__device__ __forceinline__ void inverse3(const double m[9], double o[9])
{
#define M(i, j) m[3 * (i) + (j)]
#define COF(i, j) (M(((i) + 1) % 3, ((j) + 1) % 3) * M(((i) + 2) % 3, ((j) + 2) % 3) - M(((i) + 1) % 3, ((j) + 2) % 3) * M(((i) + 2) % 3, ((j) + 1) % 3))
    const double c0 = COF(0, 0), c1 = COF(1, 0), c2 = COF(2, 0);
    const double det = (c0 * M(0, 0) + c1 * M(1, 0)) + c2 * M(2, 0);
    const double invdet = 1.0 / det;
    o[0] = c0 * invdet; o[1] = c1 * invdet; o[2] = c2 * invdet;
    o[3] = COF(0, 1) * invdet; o[4] = COF(1, 1) * invdet; o[5] = COF(2, 1) * invdet;
    o[6] = COF(0, 2) * invdet; o[7] = COF(1, 2) * invdet; o[8] = COF(2, 2) * invdet;
#undef COF
#undef M
}

// ------------------------------------------------------------------ g2o's Huber kernel

__device__ __forceinline__ void huber(double e, double delta, double &rho0, double &rho1)   // RobustKernelHuber::robustify
{
    const float dsqr = (float)(delta * delta);      // a float member in g2o
    if (e <= dsqr) { rho0 = e; rho1 = 1.; }
    else {
        const double sqrte = sqrt(e);
        rho0 = 2 * sqrte * delta - dsqr;
        rho1 = delta / sqrte;
    }
}

// ------------------------------------------------------------------ Eigen's LDLT

// What ldlt_solve does when no diagonal entry is > 0 in magnitude at step 0 -- an all-zero diagonal, or a matrix of NaN:
//   AsEigen     Eigen 3.3's "the entire diagonal is zero" exit: ZeroSign, identity transpositions, the matrix as it is, and the
//               solve runs on it.  A zero matrix gives x = 0 (D^-1 = 0); a NaN matrix gives x = NaN.  OptimizeSim3 (N = 7) uses it.
//   ReturnZero  x = 0 and isPositive() at once: the same for a zero matrix, but x = 0 for a NaN matrix too, where Eigen gives NaN.
//               PoseOptimization (N = 6) uses it, as its restatement does.
// The two solvers keep the behaviour each was written and tested with; making PoseOptimization follow Eigen is a change of its
// results on NaN input and is not made here.
enum class LdltZeroDiagonal { AsEigen, ReturnZero };

// Eigen::LDLT (Eigen 3.3 ldlt_inplace: diagonal pivoting, lower triangle) + solve; returns isPositive().  Every loop has constant
// bounds and the pivot swaps are selects over the constant candidates, so the matrix stays in registers (a dynamic index would put
// it in scratch memory, on the serial path of every trial).
template <int N, LdltZeroDiagonal ZERO_DIAGONAL>
__device__ inline bool ldlt_solve(double (&m)[N * N], const double (&b)[N], double (&x)[N])
{
    int tr[N];
    int sign = 0;   // 0 ZeroSign, 1 PositiveSemiDef, 2 NegativeSemiDef, 3 Indefinite
    double temp[N];
#define L(i, j) m[N * (i) + (j)]
    bool zero_diagonal = false;     // AsEigen: the exit at k = 0 was taken
    ORBM_UNROLL for (int k = 0; k < N; ++k) {
        if (zero_diagonal) { tr[k] = k; continue; }
        int big = k;
        double bv = fabs(L(k, k));
        ORBM_UNROLL for (int j = k + 1; j < N; ++j) {
            const double f = fabs(L(j, j));
            if (f > bv) { big = j; bv = f; }
        }
        tr[k] = big;
        ORBM_UNROLL for (int c = k + 1; c < N; ++c) {
            if (big != c) continue;
            ORBM_UNROLL for (int j = 0; j < k; ++j) { const double s = L(k, j); L(k, j) = L(c, j); L(c, j) = s; }
            ORBM_UNROLL for (int i = c + 1; i < N; ++i) { const double s = L(i, k); L(i, k) = L(i, c); L(i, c) = s; }
            { const double s = L(k, k); L(k, k) = L(c, c); L(c, c) = s; }
            ORBM_UNROLL for (int i = k + 1; i < c; ++i) { const double s = L(i, k); L(i, k) = L(c, i); L(c, i) = s; }
        }
        if (k > 0) {
            ORBM_UNROLL for (int j = 0; j < k; ++j) temp[j] = L(j, j) * L(k, j);
            double s = L(k, 0) * temp[0];
            ORBM_UNROLL for (int j = 1; j < k; ++j) s = s + L(k, j) * temp[j];
            L(k, k) -= s;
            ORBM_UNROLL for (int i = k + 1; i < N; ++i) {
                double a = L(i, 0) * temp[0];
                ORBM_UNROLL for (int j = 1; j < k; ++j) a = a + L(i, j) * temp[j];
                L(i, k) -= a;
            }
        }
        const double akk = L(k, k);
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            if (ZERO_DIAGONAL == LdltZeroDiagonal::ReturnZero) { ORBM_UNROLL for (int j = 0; j < N; ++j) x[j] = 0.0; return true; }
            zero_diagonal = true;
            continue;
        }
        if (valid)
            ORBM_UNROLL for (int i = k + 1; i < N; ++i) L(i, k) /= akk;
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
    ORBM_UNROLL for (int i = 0; i < N; ++i) y[i] = b[i];
    ORBM_UNROLL for (int k = 0; k < N; ++k)
        ORBM_UNROLL for (int c = k + 1; c < N; ++c)
            if (tr[k] == c) { const double s = y[k]; y[k] = y[c]; y[c] = s; }
    ORBM_UNROLL for (int i = 0; i < N; ++i) ORBM_UNROLL for (int j = 0; j < i; ++j) y[i] -= L(i, j) * y[j];
    ORBM_UNROLL for (int i = 0; i < N; ++i) y[i] = (fabs(L(i, i)) > 2.2250738585072014e-308) ? y[i] / L(i, i) : 0.0;
    ORBM_UNROLL for (int i = N - 1; i >= 0; --i) ORBM_UNROLL for (int j = i + 1; j < N; ++j) y[i] -= L(j, i) * y[j];
    ORBM_UNROLL for (int k = N - 1; k >= 0; --k)
        ORBM_UNROLL for (int c = k + 1; c < N; ++c)
            if (tr[k] == c) { const double s = y[k]; y[k] = y[c]; y[c] = s; }
    ORBM_UNROLL for (int i = 0; i < N; ++i) x[i] = y[i];
#undef L
    return true;
}

// ------------------------------------------------------------------ fixed-order wave and block reductions

__device__ __forceinline__ double wave_sum(double v)    // the butterfly: every lane ends with the wave's sum
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Sum of every v[j] over the block's NW waves: wave butterfly, then the waves in order.  red: NW rows of NS >= NV doubles in LDS.
template <int NV, int NW, int NS>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*red)[NS])
{
    static_assert(NV <= NS, "a row of red holds every value");
    for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
    if (NW == 1) return;
    __syncthreads();                                        // the previous reduction's readers are done with red
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
        for (int j = 0; j < NV; ++j) red[w][j] = v[j];
    __syncthreads();
    for (int j = 0; j < NV; ++j) {
        double s = red[0][j];
        ORBM_UNROLL for (int k = 1; k < NW; ++k) s = s + red[k][j];
        v[j] = s;
    }
}

template <int NW>
__device__ __forceinline__ int block_sum_int(int v, int *ired)     // ired: NW ints in LDS
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (NW == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = ired[0];
    ORBM_UNROLL for (int k = 1; k < NW; ++k) s += ired[k];
    return s;
}

} // namespace orbm_detail
