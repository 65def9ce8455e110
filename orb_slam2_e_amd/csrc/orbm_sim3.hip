// orbm_sim3.hip -- Sim3Solver (src/Sim3Solver.cc) on the device: every RANSAC hypothesis of up to 64 candidate keyframes in one call.
//
// The reference draws three indices per iteration from a freshly reset list (:163-177), so no iteration depends on an earlier one:
// the caller draws the triples of all iterations first, orbm_sim3_hypotheses evaluates them -- ComputeSim3 (:226-337) and
// CheckInliers (:340-364) per triple -- and what iterate (:140-207) returns is a fold over the inlier counts, run by the caller
// (include/orbslam_hip.hpp: Sim3Solver).  Two launches on one leased workspace's stream, one staged upload, one host wait:
//   k_sim3_prepare      per problem, once: X3Dc1/2 = Rcw * Xw + tcw (:95, :98), the self-projections P1im1 / P2im2 (:108-109) and the
//                       integer thresholds mvnMaxError1/2 (:87-88), written to the workspace
//   k_sim3_hypotheses   one wave per (problem, hypothesis): every lane computes ComputeSim3 of the triple from the same inputs (the
//                       same bits in every lane: no broadcast, no barrier), then the lanes stride over the n correspondences, each
//                       with both projections and both comparisons; __ballot words are the inlier mask, their popcounts the count.
// The arithmetic is the reference's float / double order op by op with OpenCV 3.4's cv::Mat semantics as tests/sim3_oracle.c lists
// them (unpinned like every OpenCV primitive here): float row sums of the 3 x 3 products, float scales, norm / dot in
// double, cv::eigen = JacobiImpl_<float> with its pivot bookkeeping, cv::Rodrigues in double.  No float atomics; every sum has a
// fixed order; -ffp-contract=off.
#include <atomic>

#include "orbm_internal.h"

using namespace orbm_detail;

namespace {

constexpr int SIM3_MAX_P = 64, SIM3_MAX_N = 8192, SIM3_MAX_H = 1024;

// One problem of a call, staged with the inputs.  o_*: byte offsets in the workspace.
struct Sim3Dev {
    unsigned o_X1w, o_X2w, o_oct1, o_oct2, o_tri;                    // staged inputs
    unsigned o_Xc1, o_Xc2, o_P1, o_P2, o_max1, o_max2;               // written by k_sim3_prepare
    unsigned o_mask;                                                 // result: [H][(n + 63) / 64] 64-bit words
    int n, H, fix_scale, hyp0;                                       // hyp0: index of the problem's first hypothesis in the call
    float R1[9], t1[3], R2[9], t2[3];                                // Tcw1, Tcw2
    float cam1[4], cam2[4];                                          // fx, fy, cx, cy
};

__device__ __forceinline__ float row3(const float *R, int r, float b0, float b1, float b2) { return R[3 * r] * b0 + R[3 * r + 1] * b1 + R[3 * r + 2] * b2; }
// gemm's d = float(double(t) * alpha + double(c) * beta)
__device__ __forceinline__ float gemm_out(float t, double alpha, float c, double beta) { return (float)((double)t * alpha + (double)c * beta); }

// FromCameraToImage (:405-423) / the tail of Project (:397-401); no depth test
__device__ __forceinline__ void to_image(float X, float Y, float Z, const float *cam, float &u, float &v)
{
    const float invz = 1 / Z;
    const float x = X * invz, y = Y * invz;
    u = cam[0] * x + cam[2]; v = cam[1] * y + cam[3];
}

__global__ __launch_bounds__(MT) void k_sim3_prepare(const Sim3Dev *__restrict__ probs, char *__restrict__ ws, const float *__restrict__ sigma2)
{
    const Sim3Dev &d = probs[blockIdx.y];
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= d.n || d.H == 0) return;
    const float *a = reinterpret_cast<const float *>(ws + d.o_X1w) + 3 * i, *b = reinterpret_cast<const float *>(ws + d.o_X2w) + 3 * i;
    float *c1 = reinterpret_cast<float *>(ws + d.o_Xc1) + 3 * i, *c2 = reinterpret_cast<float *>(ws + d.o_Xc2) + 3 * i;
    float x1[3], x2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        x1[r] = gemm_out(row3(d.R1, r, a[0], a[1], a[2]), 1.0, d.t1[r], 1.0);
        x2[r] = gemm_out(row3(d.R2, r, b[0], b[1], b[2]), 1.0, d.t2[r], 1.0);
        c1[r] = x1[r]; c2[r] = x2[r];
    }
    float u, v;
    to_image(x1[0], x1[1], x1[2], d.cam1, u, v);
    reinterpret_cast<float2 *>(ws + d.o_P1)[i] = make_float2(u, v);
    to_image(x2[0], x2[1], x2[2], d.cam2, u, v);
    reinterpret_cast<float2 *>(ws + d.o_P2)[i] = make_float2(u, v);
    // :87-88: 9.210 * sigma2 in double, truncated into a size_t; the comparison of :356 converts it to float
    const int l1 = reinterpret_cast<const int *>(ws + d.o_oct1)[i], l2 = reinterpret_cast<const int *>(ws + d.o_oct2)[i];
    reinterpret_cast<float *>(ws + d.o_max1)[i] = (float)(unsigned long long)(9.210 * (double)sigma2[l1]);
    reinterpret_cast<float *>(ws + d.o_max2)[i] = (float)(unsigned long long)(9.210 * (double)sigma2[l2]);
}

// ---- cv::eigen of the 4 x 4 symmetric float matrix: JacobiImpl_<float> (OpenCV 3.4 modules/core/src/lapack.cpp).  The pivot (k, l)
// is the same in every lane; its rotation is one of six instantiations with constant indices, chosen by a scalar branch, so A, W,
// V, indR and indC stay in registers.
__device__ __forceinline__ float cv_hypotf(float a, float b)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}

struct Eig4 {
    float A[16], W[4], V[16];
    int indR[4], indC[4];
};

template <int IDX> __device__ __forceinline__ void eig_track(Eig4 &e)
{
    if (IDX < 3) {
        int m = IDX + 1;
        float mv = fabsf(e.A[4 * IDX + m]);
#pragma unroll
        for (int i = IDX + 2; i < 4; ++i) { const float val = fabsf(e.A[4 * IDX + i]); if (mv < val) { mv = val; m = i; } }
        e.indR[IDX] = m;
    }
    if (IDX > 0) {
        int m = 0;
        float mv = fabsf(e.A[IDX]);
#pragma unroll
        for (int i = 1; i < IDX; ++i) { const float val = fabsf(e.A[4 * i + IDX]); if (mv < val) { mv = val; m = i; } }
        e.indC[IDX] = m;
    }
}

__device__ __forceinline__ void eig_rot(float &v0, float &v1, float c, float s)
{
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c;
}

template <int K, int L> __device__ __forceinline__ void eig_rotate(Eig4 &e, float p)
{
    const float y = (float)((double)(e.W[L] - e.W[K]) * 0.5);
    float t = fabsf(y) + cv_hypotf(p, y);
    float s = cv_hypotf(p, t);
    const float c = t / s;
    s = p / s; t = (p / t) * p;
    if (y < 0) { s = -s; t = -t; }
    e.A[4 * K + L] = 0;
    e.W[K] -= t;
    e.W[L] += t;
#pragma unroll
    for (int i = 0; i < K; ++i) eig_rot(e.A[4 * i + K], e.A[4 * i + L], c, s);
#pragma unroll
    for (int i = K + 1; i < L; ++i) eig_rot(e.A[4 * K + i], e.A[4 * i + L], c, s);
#pragma unroll
    for (int i = L + 1; i < 4; ++i) eig_rot(e.A[4 * K + i], e.A[4 * L + i], c, s);
#pragma unroll
    for (int i = 0; i < 4; ++i) eig_rot(e.V[4 * K + i], e.V[4 * L + i], c, s);
    eig_track<K>(e);
    eig_track<L>(e);
}

// q[4] = evec.row(0): the row of the largest eigenvalue (the first of equal ones, as the descending sort leaves it)
__device__ __forceinline__ void eigen4_row0(const float *N, float *q)
{
    Eig4 e;
#pragma unroll
    for (int i = 0; i < 16; ++i) { e.A[i] = N[i]; e.V[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) e.W[k] = e.A[5 * k];
    e.indR[3] = 0; e.indC[0] = 0;
    eig_track<0>(e); eig_track<1>(e); eig_track<2>(e); eig_track<3>(e);
    for (int iters = 0; iters < 4 * 4 * 30; ++iters) {
        // the pivot: the largest of the tracked row maxima, then of the tracked column maxima
        int k = 0, l;
        float mv = fabsf(e.indR[0] == 1 ? e.A[1] : e.indR[0] == 2 ? e.A[2] : e.A[3]);
        { const float val = fabsf(e.indR[1] == 2 ? e.A[6] : e.A[7]); if (mv < val) { mv = val; k = 1; } }
        { const float val = fabsf(e.A[11]); if (mv < val) { mv = val; k = 2; } }
        l = k == 0 ? e.indR[0] : k == 1 ? e.indR[1] : 3;
        { const float val = fabsf(e.A[1]); if (mv < val) { mv = val; k = 0; l = 1; } }
        { const float val = fabsf(e.indC[2] == 0 ? e.A[2] : e.A[6]); if (mv < val) { mv = val; k = e.indC[2]; l = 2; } }
        { const float val = fabsf(e.indC[3] == 0 ? e.A[3] : e.indC[3] == 1 ? e.A[7] : e.A[11]); if (mv < val) { mv = val; k = e.indC[3]; l = 3; } }
        const int kl = __builtin_amdgcn_readfirstlane(4 * k + l);           // the same in every lane: a scalar branch
        float p;
        switch (kl) {
        case 1: p = e.A[1]; break;
        case 2: p = e.A[2]; break;
        case 3: p = e.A[3]; break;
        case 6: p = e.A[6]; break;
        case 7: p = e.A[7]; break;
        default: p = e.A[11]; break;
        }
        if (fabsf(p) <= 1.1920929e-07f) break;                             // FLT_EPSILON
        switch (kl) {
        case 1: eig_rotate<0, 1>(e, p); break;
        case 2: eig_rotate<0, 2>(e, p); break;
        case 3: eig_rotate<0, 3>(e, p); break;
        case 6: eig_rotate<1, 2>(e, p); break;
        case 7: eig_rotate<1, 3>(e, p); break;
        default: eig_rotate<2, 3>(e, p); break;
        }
    }
    int m = 0;
    float wm = e.W[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) if (wm < e.W[i]) { wm = e.W[i]; m = i; }
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = m == 0 ? e.V[c] : m == 1 ? e.V[4 + c] : m == 2 ? e.V[8 + c] : e.V[12 + c];
}

// cv::Rodrigues, vector -> matrix, in double (cvRodrigues2); a NaN vector gives a NaN matrix
__device__ __forceinline__ void rodrigues(const float *v, float *R)
{
    double rx = v[0], ry = v[1], rz = v[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < 2.220446049250313e-16) {                                   // DBL_EPSILON
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (float)((c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * r_x[i]);
}

// ComputeCentroid (:215-224): p[i][r] = coordinate r of point i; Pr[r][i], C[r]
__device__ __forceinline__ void centroid(const float (&p)[3][3], float (&Pr)[3][3], float (&C)[3])
{
    const float third = (float)(1.0 / 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float sum = (p[0][r] + p[2][r]) + p[1][r];                   // cv::reduce of a row of three
        C[r] = sum * third + 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) Pr[r][i] = p[i][r] - C[r];
    }
}

// ComputeSim3 (:226-337).  T12 / T21 as 3 x 4 (the last row of both is 0 0 0 1).
__device__ __forceinline__ void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], int fix_scale, float (&T12)[12], float (&T21)[12],
                                             float (&R)[9], float &s12)
{
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3], N[16], q[4], vec[3], P3[3][3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = gemm_out(Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1] + Pr2[r][2] * Pr1[c][2], 1.0, 0.0f, 0.0);
    // N11 .. N44 are doubles formed from float sums, stored back into a float matrix (:247-265)
    const double N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0],
                 N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2],
                 N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
#pragma unroll
    for (int k = 0; k < 16; ++k) N[k] = (float)Nd[k];
    eigen4_row0(N, q);
    vec[0] = q[1]; vec[1] = q[2]; vec[2] = q[3];
    const double nrm = sqrt((double)vec[0] * vec[0] + (double)vec[1] * vec[1] + (double)vec[2] * vec[2]);
    const double ang = atan2(nrm, (double)q[0]);                                          // :278
    const double alpha = (2 * ang) * (1. / nrm);                                          // :280; 0 / 0 for the identity: NaN from here on
#pragma unroll
    for (int k = 0; k < 3; ++k) vec[k] = vec[k] * (float)alpha + 0.0f;
    rodrigues(vec, R);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) P3[r][c] = gemm_out(R[3 * r] * Pr2[0][c] + R[3 * r + 1] * Pr2[1][c] + R[3 * r + 2] * Pr2[2][c], 1.0, 0.0f, 0.0);
    float s = 1.0f;
    if (!fix_scale) {
        // Mat::dot: double products in groups of four; den: a double sum of float squares, row by row
        double nom = 0, den = 0;
        nom += (double)Pr1[0][0] * P3[0][0] + (double)Pr1[0][1] * P3[0][1] + (double)Pr1[0][2] * P3[0][2] + (double)Pr1[1][0] * P3[1][0];
        nom += (double)Pr1[1][1] * P3[1][1] + (double)Pr1[1][2] * P3[1][2] + (double)Pr1[2][0] * P3[2][0] + (double)Pr1[2][1] * P3[2][1];
        nom += (double)Pr1[2][2] * P3[2][2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) { const float sq = P3[r][c] * P3[r][c]; den += sq; }
        s = (float)(nom / den);
    }
    float t12[3], sRinv[9];
    const float sf = (float)(double)s, inv = (float)(1.0 / s);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t12[r] = gemm_out(row3(R, r, O2[0], O2[1], O2[2]), -(double)s, O1[r], 1.0);       // O1 - s * R * O2: one gemm
#pragma unroll
        for (int c = 0; c < 3; ++c) { T12[4 * r + c] = R[3 * r + c] * sf + 0.0f; sRinv[3 * r + c] = R[3 * c + r] * inv + 0.0f; }
        T12[4 * r + 3] = t12[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T21[4 * r + c] = sRinv[3 * r + c];
        T21[4 * r + 3] = gemm_out(row3(sRinv, r, t12[0], t12[1], t12[2]), -1.0, 0.0f, 0.0);
    }
    s12 = s;
}

// Project (:382-403) of one point through a 3 x 4 transformation
__device__ __forceinline__ void project(const float (&T)[12], const float *X, const float *cam, float &u, float &v)
{
    float P[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = gemm_out(T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2], 1.0, T[4 * r + 3], 1.0);
    to_image(P[0], P[1], P[2], cam, u, v);
}

__global__ __launch_bounds__(MT) void k_sim3_hypotheses(const Sim3Dev *__restrict__ probs, int P, int total, char *__restrict__ ws,
                                                        orbm_sim3_hypothesis *__restrict__ hyp)
{
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MT / 64) + (threadIdx.x >> 6)));   // the wave's hypothesis in the call
    if (g >= total) return;
    int p = 0;
    for (int j = 1; j < P; ++j) if (probs[j].hyp0 <= g) p = j;        // hyp0 ascends; problems without hypotheses share their successor's
    const Sim3Dev &d = probs[p];
    const int h = g - d.hyp0, n = d.n;
    const float *Xc1 = reinterpret_cast<const float *>(ws + d.o_Xc1), *Xc2 = reinterpret_cast<const float *>(ws + d.o_Xc2);
    const int *tri = reinterpret_cast<const int *>(ws + d.o_tri) + 3 * h;
    float P1[3][3], P2[3][3], T12[12], T21[12], R[9], s12;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int idx = tri[k];                                        // inside [0, n): checked on the host before the launch
#pragma unroll
        for (int r = 0; r < 3; ++r) { P1[k][r] = Xc1[3 * idx + r]; P2[k][r] = Xc2[3 * idx + r]; }
    }
    compute_sim3(P1, P2, d.fix_scale, T12, T21, R, s12);
    if (lane == 0) {
        orbm_sim3_hypothesis &o = hyp[g];
#pragma unroll
        for (int k = 0; k < 12; ++k) o.T12[k] = T12[k];
        o.T12[12] = 0.0f; o.T12[13] = 0.0f; o.T12[14] = 0.0f; o.T12[15] = 1.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) o.R12[k] = R[k];
        o.t12[0] = T12[3]; o.t12[1] = T12[7]; o.t12[2] = T12[11];
        o.s12 = s12;
    }
    // CheckInliers (:340-364): lane = correspondence, 64 per round
    const float2 *P1im1 = reinterpret_cast<const float2 *>(ws + d.o_P1), *P2im2 = reinterpret_cast<const float2 *>(ws + d.o_P2);
    const float *max1 = reinterpret_cast<const float *>(ws + d.o_max1), *max2 = reinterpret_cast<const float *>(ws + d.o_max2);
    const int words = (n + 63) >> 6;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(ws + d.o_mask) + (size_t)h * words;
    int count = 0;
    for (int w = 0; w < words; ++w) {
        const int i = 64 * w + lane;
        bool in = false;
        if (i < n) {
            float u, v;
            project(T12, Xc2 + 3 * i, d.cam1, u, v);                  // vP2im1
            const float2 a = P1im1[i];
            const float d1x = a.x - u, d1y = a.y - v;
            project(T21, Xc1 + 3 * i, d.cam2, u, v);                  // vP1im2
            const float2 b = P2im2[i];
            const float d2x = u - b.x, d2y = v - b.y;
            const float err1 = (float)((double)d1x * d1x + (double)d1y * d1y), err2 = (float)((double)d2x * d2x + (double)d2y * d2y);
            in = err1 < max1[i] && err2 < max2[i];
        }
        const unsigned long long word = __ballot(in);                 // bits past n are 0
        count += __popcll(word);                                       // the same in every lane
        if (lane == 0) mask[w] = word;
    }
    if (lane == 0) hyp[g].ninliers = count;
}

std::atomic<int> g_last_sim3_waits{0};     // host waits of the last orbm_sim3_hypotheses call of this process

} // namespace

extern "C" {

int orbm_sim3_hypotheses(const orbm_sim3_problem *problems, int P, const float *level_sigma2, int nlevels, orbm_sim3_hypothesis *hyp,
                         void *inliers)
{
    g_last_sim3_waits.store(0, std::memory_order_relaxed);
    if (P < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (P > SIM3_MAX_P) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 64 problems in one call");
    if (P && !problems) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    int total = 0, max_n = 0;
    for (int p = 0; p < P; ++p) {
        const orbm_sim3_problem &q = problems[p];
        if (q.n < 0 || q.H < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        if (q.n > SIM3_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 correspondences in a problem");
        if (q.H > SIM3_MAX_H) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,024 hypotheses in a problem");
        if (q.H == 0) continue;
        if (q.n < 3) ORBX_FAIL(ORBX_ERR_ARG, "a hypothesis needs three correspondences");
        if (!q.X1w || !q.X2w || !q.octave1 || !q.octave2 || !q.Tcw1 || !q.Tcw2 || !q.triples || !level_sigma2 || nlevels < 1 || !hyp || !inliers)
            ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        for (int i = 0; i < 3 * q.H; i += 3) {
            const int32_t a = q.triples[i], b = q.triples[i + 1], c = q.triples[i + 2];
            if (a < 0 || a >= q.n || b < 0 || b >= q.n || c < 0 || c >= q.n) ORBX_FAIL(ORBX_ERR_ARG, "triple index out of range");
            if (a == b || a == c || b == c) ORBX_FAIL(ORBX_ERR_ARG, "a triple repeats an index");
        }
        if (!octaves_in_range(q, nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
        total += q.H;
        max_n = std::max(max_n, (int)q.n);
    }
    if (total == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    std::vector<Sim3Dev> dev((size_t)P);
    StagedCall sc;
    const size_t o_dev = sc.in(dev.data(), sizeof(Sim3Dev) * (size_t)P), o_sg = sc.in(level_sigma2, sizeof(float) * (size_t)nlevels);
    for (int p = 0; p < P; ++p) {
        const orbm_sim3_problem &q = problems[p];
        Sim3Dev &d = dev[p];
        memset(&d, 0, sizeof(d));
        d.n = q.n; d.H = q.H; d.fix_scale = q.fix_scale ? 1 : 0;
        if (q.H == 0) continue;
        stage_two_keyframes(sc, q, d);
        d.o_tri = (unsigned)sc.in(q.triples, sizeof(int32_t) * 3 * (size_t)q.H);
    }
    for (int p = 0; p < P; ++p) {
        Sim3Dev &d = dev[p];
        if (d.H == 0) continue;
        const size_t n = (size_t)d.n;
        d.o_Xc1 = (unsigned)sc.scratch(sizeof(float) * 3 * n); d.o_Xc2 = (unsigned)sc.scratch(sizeof(float) * 3 * n);
        d.o_P1 = (unsigned)sc.scratch(sizeof(float) * 2 * n); d.o_P2 = (unsigned)sc.scratch(sizeof(float) * 2 * n);
        d.o_max1 = (unsigned)sc.scratch(sizeof(float) * n); d.o_max2 = (unsigned)sc.scratch(sizeof(float) * n);
    }
    const size_t o_hyp = sc.out(sizeof(orbm_sim3_hypothesis) * (size_t)total);
    int h0 = 0;
    for (int p = 0; p < P; ++p) {
        Sim3Dev &d = dev[p];
        d.hyp0 = h0;
        h0 += d.H;
        if (d.H) d.o_mask = (unsigned)sc.out(sizeof(uint64_t) * (size_t)d.H * (size_t)((d.n + 63) / 64));
    }
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_sim3_prepare, dim3((unsigned)((max_n + MT - 1) / MT), (unsigned)P), dim3(MT), 0, sc.stream(), sc.d<const Sim3Dev>(o_dev),
                       sc.d<char>(0), sc.d<const float>(o_sg));
    ORBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((total + MT / 64 - 1) / (MT / 64))), dim3(MT), 0, sc.stream(), sc.d<const Sim3Dev>(o_dev), P,
                       total, sc.d<char>(0), sc.d<orbm_sim3_hypothesis>(o_hyp));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_sim3_waits.store(sc.waits, std::memory_order_relaxed);      // counted where the stream is waited for
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(hyp, sc.r<orbm_sim3_hypothesis>(o_hyp), sizeof(orbm_sim3_hypothesis) * (size_t)total);
    uint64_t *out = static_cast<uint64_t *>(inliers);
    for (int p = 0; p < P; ++p) {
        const Sim3Dev &d = dev[p];
        const size_t words = (size_t)d.H * (size_t)((d.n + 63) / 64);
        if (d.H) memcpy(out, sc.r<uint64_t>(d.o_mask), sizeof(uint64_t) * words);
        out += words;
    }
    return ORBX_OK;
}

int orbm_debug_last_sim3_waits(void) { return g_last_sim3_waits.load(std::memory_order_relaxed); }

} // extern "C"
