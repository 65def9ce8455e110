// orbm_svd.h -- cv::SVDecomp / cv::SVD::compute of a float matrix as OpenCV 3.4 computes it: JacobiSVDImpl_<float>
// (modules/core/src/lapack.cpp) in its general (m, n, n1) form, for the host and the device.  OpenCV is not available to this
// project, so like every OpenCV primitive here the restatement is unpinned; tests/test_cpu_init.py holds it to first
// principles and to tests/init_oracle.c.
//
// How _SVDcompute drives the routine for a src of `rows` x `cols`:
//   rows >= cols   At = src.t() (cols rows of length rows), M = rows, N = cols; vt = Vt (the accumulated rotations, N x N),
//                  u = At.t() after the tail; with FULL_UV n1 = rows, else n1 = cols (the rows N .. n1-1 of At only reach u)
//   rows <  cols   the roles swap: At = src as it is (rows rows of length cols), M = cols, N = rows, n1 = cols (FULL_UV);
//                  vt = At after the tail (n1 rows), u = Vt.t()
// The routine: one-sided Jacobi rotations over the N (N - 1) / 2 pairs of rows of At, the products of two rows and the new squared
// norms accumulated in double over k ascending, eps = 2 FLT_EPSILON, the hypot / sqrt branch pair, until a sweep applies no
// rotation (at most max(M, 30) sweeps); singular values = sqrt of the squared row norms, sorted descending by a selection sort
// that swaps the rows of At and Vt; then the tail: row i < n1 of At is scaled by (float)(1 / sd), and a row whose singular value
// is <= FLT_MIN (every row i >= N) is first replaced by a vector of +-(float)(1. / M) with signs from cv::RNG(0x12345678), with
// the earlier rows projected out twice, up to 100 times.
//
// Every array index below is a constant once the loops are unrolled (the sort's dynamic row is met by a uniform branch per
// candidate row), so on the device At, Vt and W stay in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#include <utility>

#if defined(__HIPCC__)
#define ORBM_SVD_HD __host__ __device__ __forceinline__
#else
#define ORBM_SVD_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ORBM_SVD_UNROLL _Pragma("unroll")      // the device code needs constant indices; the host code is left to the compiler
#else
#define ORBM_SVD_UNROLL
#endif

namespace orbm_svd {

// cv::RNG::next(): multiply-with-carry
ORBM_SVD_HD unsigned rng_next(uint64_t &state)
{
    state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
}

template <int M> ORBM_SVD_HD void swap_rows(float (&a)[M], float (&b)[M])
{
ORBM_SVD_UNROLL
    for (int k = 0; k < M; ++k) { const float t = a[k]; a[k] = b[k]; b[k] = t; }
}

// The routine's tail for row I (a template parameter, so that the loop over the earlier rows has a constant bound): the row whose
// singular value is <= FLT_MIN is made afresh, then every row is scaled by (float)(1 / sd).  The RNG state runs on across rows.
template <int M, int N, int N1, int I>
ORBM_SVD_HD void tail_row(float (&At)[N1][M], const double (&W)[N], uint64_t &rng)
{
    const float eps = 1.1920928955078125e-7f * 2;
    const double minval = 1.17549435082228750797e-38;    // FLT_MIN
    double sd = I < N ? W[I < N ? I : 0] : 0;
    for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
        const float val0 = (float)(1. / M);
ORBM_SVD_UNROLL
        for (int k = 0; k < M; ++k) At[I][k] = (rng_next(rng) & 256) != 0 ? val0 : -val0;
ORBM_SVD_UNROLL
        for (int it = 0; it < 2; ++it)
ORBM_SVD_UNROLL
            for (int j = 0; j < I; ++j) {
                sd = 0;
ORBM_SVD_UNROLL
                for (int k = 0; k < M; ++k) sd += At[I][k] * At[j][k];               // a float product into the double sum
                float asum = 0;
ORBM_SVD_UNROLL
                for (int k = 0; k < M; ++k) {
                    const float t = (float)(At[I][k] - sd * At[j][k]);
                    At[I][k] = t;
                    asum += fabsf(t);
                }
                asum = asum > eps * 100 ? 1 / asum : 0;
ORBM_SVD_UNROLL
                for (int k = 0; k < M; ++k) At[I][k] *= asum;
            }
        sd = 0;
ORBM_SVD_UNROLL
        for (int k = 0; k < M; ++k) { const float t = At[I][k]; sd += (double)t * t; }
        sd = sqrt(sd);
    }
    const float s = (float)(sd > minval ? 1 / sd : 0.);
ORBM_SVD_UNROLL
    for (int k = 0; k < M; ++k) At[I][k] *= s;
}

template <int M, int N, int N1, int... I>
ORBM_SVD_HD void tail_rows(float (&At)[N1][M], const double (&W)[N], uint64_t &rng, std::integer_sequence<int, I...>)
{
    (tail_row<M, N, N1, I>(At, W, rng), ...);
}

// JacobiSVDImpl_<float>(At, _W = w, Vt, m = M, n = N, n1 = N1, minval = FLT_MIN, eps = 2 FLT_EPSILON).  At: N1 rows of length M,
// the rows N .. N1-1 zero on entry.  WANT_VT = false leaves Vt alone (a caller that reads only At: the rotations of Vt feed
// nothing else); TAIL = false stops after the sort (a caller that reads only Vt and w: the tail writes At alone).
template <int M, int N, int N1, bool WANT_VT, bool TAIL>
ORBM_SVD_HD void jacobi_svd(float (&At)[N1][M], float (&w)[N], float (&Vt)[N][N])
{
    static_assert(N1 >= N, "n1 >= n");
    const float eps = 1.1920928955078125e-7f * 2;        // FLT_EPSILON * 2
    double W[N];
ORBM_SVD_UNROLL
    for (int i = 0; i < N; ++i) {
        double sd = 0;
ORBM_SVD_UNROLL
        for (int k = 0; k < M; ++k) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sd;
        if (WANT_VT) {
ORBM_SVD_UNROLL
            for (int k = 0; k < N; ++k) Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
    }
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
ORBM_SVD_UNROLL
        for (int i = 0; i < N - 1; ++i)
ORBM_SVD_UNROLL
            for (int j = i + 1; j < N; ++j) {
                double a = W[i], p = 0, b = W[j];
ORBM_SVD_UNROLL
                for (int k = 0; k < M; ++k) p += (double)At[i][k] * At[j][k];
                if (!(fabs(p) <= eps * sqrt((double)a * b))) {
                    p *= 2;
                    const double beta = a - b, gamma = hypot((double)p, beta);
                    float c, s;
                    if (beta < 0) {
                        const double delta = (gamma - beta) * 0.5;
                        s = (float)sqrt(delta / gamma);
                        c = (float)(p / (gamma * s * 2));
                    } else {
                        c = (float)sqrt((gamma + beta) / (gamma * 2));
                        s = (float)(p / (gamma * c * 2));
                    }
                    a = b = 0;
ORBM_SVD_UNROLL
                    for (int k = 0; k < M; ++k) {
                        const float t0 = c * At[i][k] + s * At[j][k];
                        const float t1 = -s * At[i][k] + c * At[j][k];
                        At[i][k] = t0; At[j][k] = t1;
                        a += (double)t0 * t0; b += (double)t1 * t1;
                    }
                    W[i] = a; W[j] = b;
                    changed = true;
                    if (WANT_VT) {
ORBM_SVD_UNROLL
                        for (int k = 0; k < N; ++k) {
                            const float t0 = c * Vt[i][k] + s * Vt[j][k];
                            const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                            Vt[i][k] = t0; Vt[j][k] = t1;
                        }
                    }
                }
            }
        if (!changed) break;
    }
ORBM_SVD_UNROLL
    for (int i = 0; i < N; ++i) {
        double sd = 0;
ORBM_SVD_UNROLL
        for (int k = 0; k < M; ++k) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    // the selection sort, descending: j = the first row holding the largest of W[i ..], found as `W[j] < W[k]` finds it
ORBM_SVD_UNROLL
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        double wj = W[i];
ORBM_SVD_UNROLL
        for (int k = i + 1; k < N; ++k) { const bool m = wj < W[k]; j = m ? k : j; wj = m ? W[k] : wj; }
ORBM_SVD_UNROLL
        for (int k = i + 1; k < N; ++k)
            if (j == k) {
                const double t = W[i]; W[i] = W[k]; W[k] = t;
                swap_rows<M>(At[i], At[k]);
                if (WANT_VT) swap_rows<N>(Vt[i], Vt[k]);
            }
    }
ORBM_SVD_UNROLL
    for (int i = 0; i < N; ++i) w[i] = (float)W[i];
    if (!TAIL) return;
    uint64_t rng = 0x12345678;
    tail_rows<M, N, N1>(At, W, rng, std::make_integer_sequence<int, N1>());
}

// ---- cv::Mat pieces around it, 3 x 3 float, row-major

// gemm's small-matrix case without C: the float row sum left to right, then float(double(sum) * 1.0 + 0.0 * 0.0)
ORBM_SVD_HD void gemm33(const float *A, const float *B, float *D)
{
    float out[9];
ORBM_SVD_UNROLL
    for (int r = 0; r < 3; ++r)
ORBM_SVD_UNROLL
        for (int c = 0; c < 3; ++c) {
            const float t = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
            out[3 * r + c] = (float)((double)t * 1.0 + (double)0.0f * 0.0);
        }
ORBM_SVD_UNROLL
    for (int k = 0; k < 9; ++k) D[k] = out[k];
}

// det3 of cv::determinant / cv::invert: in double from the float entries
ORBM_SVD_HD double det33(const float *m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// cv::invert, the 3 x 3 float case of DECOMP_LU: determinant and cofactors in double, one 1. / d, stored as float; all zero when d == 0
ORBM_SVD_HD void invert33(const float *S, float *Dst)
{
    double d = det33(S);
    float out[9];
    if (d != 0.) {
        d = 1. / d;
        out[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
        out[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
        out[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
        out[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
        out[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
        out[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
        out[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
        out[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
        out[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
    } else {
ORBM_SVD_UNROLL
        for (int k = 0; k < 9; ++k) out[k] = 0.0f;
    }
ORBM_SVD_UNROLL
    for (int k = 0; k < 9; ++k) Dst[k] = out[k];
}

// cv::SVDecomp(A, w, u, vt) of a 3 x 3 float matrix (FULL_UV or not: the same for a square one)
ORBM_SVD_HD void svd33(const float *A, float *w, float *u, float *vt)
{
    float At[3][3], Vt[3][3], W[3];
ORBM_SVD_UNROLL
    for (int i = 0; i < 3; ++i)
ORBM_SVD_UNROLL
        for (int k = 0; k < 3; ++k) At[i][k] = A[3 * k + i];
    jacobi_svd<3, 3, 3, true, true>(At, W, Vt);
ORBM_SVD_UNROLL
    for (int i = 0; i < 3; ++i) {
        w[i] = W[i];
ORBM_SVD_UNROLL
        for (int k = 0; k < 3; ++k) { u[3 * k + i] = At[i][k]; vt[3 * i + k] = Vt[i][k]; }
    }
}

// vt.row(8) of cv::SVDecomp of the 16 x 9 matrix whose COLUMNS are At[0..8] (ComputeH21)
ORBM_SVD_HD void svd_16x9_vt8(float (&At)[9][16], float *v)
{
    float Vt[9][9], W[9];
    jacobi_svd<16, 9, 9, true, false>(At, W, Vt);
ORBM_SVD_UNROLL
    for (int k = 0; k < 9; ++k) v[k] = Vt[8][k];
}

// vt.row(8) of cv::SVDecomp(.., FULL_UV) of the 8 x 9 matrix whose ROWS are At[0..7]; At[8] must be zero on entry (ComputeF21)
ORBM_SVD_HD void svd_8x9_vt8(float (&At)[9][9], float *v)
{
    float Vt[8][8], W[8];
    jacobi_svd<9, 8, 9, false, true>(At, W, Vt);
ORBM_SVD_UNROLL
    for (int k = 0; k < 9; ++k) v[k] = At[8][k];
}

// vt.row(3) of cv::SVD::compute of the 4 x 4 matrix whose COLUMNS are At[0..3] (Triangulate)
ORBM_SVD_HD void svd_4x4_vt3(float (&At)[4][4], float *v)
{
    float Vt[4][4], W[4];
    jacobi_svd<4, 4, 4, true, false>(At, W, Vt);
ORBM_SVD_UNROLL
    for (int k = 0; k < 4; ++k) v[k] = Vt[3][k];
}

} // namespace orbm_svd
