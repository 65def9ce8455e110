// orbm_triang.hip -- ORBmatcher::SearchForTriangulation and LocalMapping::CreateNewMapPoints for gfx950:
//   SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)   src/ORBmatcher.cc:858-1024, CheckDistEpipolarLine :341-358
//   CreateNewMapPoints                                                     src/LocalMapping.cc:281-517
// Three entry families share ONE gated candidate scan (triang_scan, templated on how KF2's features are read): the inner loop over
// explicit candidate lists and the whole function on host arrays (orbm_match_triangulation, orbm_search_for_triangulation:
// k_triang_arrays), the whole function on two resident frames (orbm_frame_search_for_triangulation: k_triang_frames), and
// k_create_points, which chains the triangulation of every neighbour keyframe behind the scan.
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "common.h"
#include "orbm_internal.h"
#include "orbx_math.h"

using namespace orbm_detail;

namespace {

// ORBmatcher::SearchForTriangulation's gated loop (src/ORBmatcher.cc:892-990 with CheckDistEpipolarLine :341-358): 16 lanes per
// keypoint of KF1; its candidates = cand[cbeg[i] .. cend[i]) of KF2 in the order the reference visits them (the members of its
// vocabulary node in KF2, one copy per node; or the caller's own lists).  The reference keeps the LAST candidate among those of
// smallest distance that pass the gates (`dist > bestDist` is non-strict, and the gates do not depend on bestDist; vbMatched2 is
// never set there, so the keypoints are independent): the minimum of dist << 16 | (0xffff - position in the list).  (One lane per
// keypoint walking its list alone was a 68-us chain of dependent loads for 2,000 keypoints.)
struct TriForm { float F12[9]; float ex, ey; int only_stereo; };

// How the scan reads a candidate of KF2: by position in a resident frame's arrays ("stereo" = the frame's right coordinate >= 0,
// mvuRight[idx] >= 0, :911 / :931; the "owns a point" mask is by feature index) ...
struct FrameKF2 {
    const SeqKp *__restrict__ kp; const int *__restrict__ perm; const uint8_t *__restrict__ hasmp;
    __device__ __forceinline__ bool owns_point(int p) const { return hasmp[perm[p]]; }
    __device__ __forceinline__ bool stereo(int p) const { return kp[p].uright >= 0; }
    __device__ __forceinline__ SeqKp record(int p) const { return kp[p]; }
};
// ... or by feature index in the caller's arrays
struct ArrayKF2 {
    const orbx_keypoint *__restrict__ kps; const uint8_t *__restrict__ hasmp; const uint8_t *__restrict__ st;
    __device__ __forceinline__ bool owns_point(int j) const { return hasmp[j]; }
    __device__ __forceinline__ bool stereo(int j) const { return st[j] != 0; }
    __device__ __forceinline__ orbx_keypoint record(int j) const { return kps[j]; }
};

// The gated candidate scan of one keypoint of KF1 (k1, descriptor a0 a1) over its list cand[k0 .. kend) of KF2, strided over the 16
// lanes of its group: this lane's smallest key, 0xffffffff = none.  The one copy of the gates (:906-985) for k_triang_frames,
// k_triang_arrays and k_create_points.
template <typename KF2>
__device__ __forceinline__ unsigned triang_scan(const SeqKp &k1, bool st1, const uint4 &a0, const uint4 &a1, const TriForm &tp, int k0, int kend,
                                                int sub, const int *__restrict__ cand, const KF2 &kf2, const uint4 *__restrict__ B,
                                                const float *__restrict__ scale2, const float *__restrict__ sigma2)
{
    unsigned key = 0xffffffffu;
    // epipolar line in the second image l = x1' F12 = [a b c]
    const float a = k1.x * tp.F12[0] + k1.y * tp.F12[3] + tp.F12[6];
    const float b = k1.x * tp.F12[1] + k1.y * tp.F12[4] + tp.F12[7];
    const float c = k1.x * tp.F12[2] + k1.y * tp.F12[5] + tp.F12[8];
    const float den = a * a + b * b;
    for (int k = k0 + sub; k < kend; k += 16) {
        const int p = cand[k];
        if (kf2.owns_point(p)) continue;
        const bool st2 = kf2.stereo(p);
        if (tp.only_stereo && !st2) continue;
        const int dist = popc256(a0, a1, B[2 * p], B[2 * p + 1]);
        if (dist > 45) continue;           // TH_LOW
        const auto k2 = kf2.record(p);
        if (!st1 && !st2) {
            const float distex = tp.ex - k2.x, distey = tp.ey - k2.y;
            if (distex * distex + distey * distey < 100 * scale2[k2.octave]) continue;
        }
        const float num = a * k2.x + b * k2.y + c;
        if (den == 0) continue;
        const float dsqr = num * num / den;
        if ((double)dsqr < 3.84 * (double)sigma2[k2.octave]) {
            const unsigned kk = ((unsigned)dist << 16) | (0xffffu - (unsigned)min(k - k0, 0xffff));
            key = kk < key ? kk : key;
        }
    }
    return key;
}

// On two resident frames: the keypoints of KF1 in its sorted order (s -> feature i = perm1[s]), candidates as positions in KF2's
// arrays.  Out, by feature index of KF1: match12 = feature index in KF2 or -1; rot = angle1 - angle2 of the pair (:994), for the
// host's histogram.
__global__ __launch_bounds__(MT) void k_triang_frames(const SeqKp *__restrict__ kp1, const uint4 *__restrict__ A, const float *__restrict__ ang1,
                                                      const int *__restrict__ perm1, int n1, const SeqKp *__restrict__ kp2,
                                                      const uint4 *__restrict__ B, const float *__restrict__ ang2, const int *__restrict__ perm2,
                                                      const int *__restrict__ cbeg, const int *__restrict__ cend, const int *__restrict__ cand,
                                                      const uint8_t *__restrict__ hasmp1, const uint8_t *__restrict__ hasmp2, TriForm tp,
                                                      const float *__restrict__ scale2, const float *__restrict__ sigma2,
                                                      int *__restrict__ match12, float *__restrict__ rot)
{
    const int s = (blockIdx.x * MT + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (s >= n1) return;                       // (whole 16-lane groups leave together)
    const int i = perm1[s];
    const SeqKp k1 = kp1[s];
    const bool st1 = k1.uright >= 0;
    unsigned key = 0xffffffffu;
    int k0 = 0;
    if (!hasmp1[i] && !(tp.only_stereo && !st1)) {
        k0 = cbeg[i];
        key = triang_scan(k1, st1, A[2 * s], A[2 * s + 1], tp, k0, cend[i], sub, cand, FrameKF2{kp2, perm2, hasmp2}, B, scale2, sigma2);
    }
    key = orbx::row_min_u32(key);
    if (sub == 0) {
        const bool hit = key != 0xffffffffu;
        const int p = hit ? cand[k0 + (int)(0xffffu - (key & 0xffffu))] : 0;
        match12[i] = hit ? perm2[p] : -1;
        rot[i] = hit ? ang1[s] - ang2[p] : 0.0f;
    }
}

// On host arrays: keypoints and candidates by feature index, "stereo" from the caller's masks.  Out [n1]: match12 = index in KF2 or
// -1; bestdist = the pair's distance, 45 (TH_LOW) for none.
__global__ __launch_bounds__(MT) void k_triang_arrays(const orbx_keypoint *__restrict__ kps1, const uint4 *__restrict__ A, int n1,
                                                      const orbx_keypoint *__restrict__ kps2, const uint4 *__restrict__ B,
                                                      const int *__restrict__ cbeg, const int *__restrict__ cend, const int *__restrict__ cand,
                                                      const uint8_t *__restrict__ hasmp1, const uint8_t *__restrict__ hasmp2,
                                                      const uint8_t *__restrict__ stereo1, const uint8_t *__restrict__ stereo2, TriForm tp,
                                                      const float *__restrict__ scale2, const float *__restrict__ sigma2,
                                                      int *__restrict__ match12, int *__restrict__ bestdist)
{
    const int i = (blockIdx.x * MT + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (i >= n1) return;                       // (whole 16-lane groups leave together)
    unsigned key = 0xffffffffu;
    int k0 = 0;
    if (!hasmp1[i] && !(tp.only_stereo && !stereo1[i])) {
        const orbx_keypoint kp1 = kps1[i];
        k0 = cbeg[i];
        key = triang_scan(SeqKp{kp1.x, kp1.y, -1.0f, kp1.octave}, stereo1[i] != 0, A[2 * i], A[2 * i + 1], tp, k0, cend[i], sub, cand,
                          ArrayKF2{kps2, hasmp2, stereo2}, B, scale2, sigma2);
    }
    key = orbx::row_min_u32(key);
    if (sub == 0) {
        const bool hit = key != 0xffffffffu;
        match12[i] = hit ? cand[k0 + (int)(0xffffu - (key & 0xffffu))] : -1;
        bestdist[i] = hit ? (int)(key >> 16) : 45;
    }
}

// ------------------------------------------------------------------------------------------------ LocalMapping::CreateNewMapPoints
// The arithmetic behind a matched pair (src/LocalMapping.cc:338-497) in the reference's float / double order, op by op.  cv::Mat
// arithmetic as restated above project_point (orbm_search_internal.h), plus (OpenCV 3.4, parity unpinned like the rest):
//   s * row - row      addWeighted with float weights: a * s + b * -1.0f
//   v / s              convertTo with a FLOAT scale: v * float(1.0 / double(s))
//   cv::SVD::compute   JacobiSVDImpl_<float> (modules/core/src/lapack.cpp) on the transposed copy: rotations of the pairs of
//                      columns of A with double column products, eps = 2 FLT_EPSILON, until a sweep applies none (at most 30),
//                      singular values sorted descending, vt.row(3)
// cos / atan2 with float operands are cosf / atan2f (using namespace std): cosf as glibc evaluates it (orbx_math.h), atan2f the
// device library's.  sqrt / hypot in double are the device library's.
struct TriPose { float Rcw[9], tcw[3], Rwc[9], Ow[3]; float fx, fy, cx, cy, invfx, invfy, mb, mbf; };
struct TriNeigh {            // one neighbour keyframe of a k_create_points launch
    const SeqKp *kp2; const uint4 *B; const int *perm2;      // the resident frame
    unsigned o_cbeg, o_cend, o_cand, o_has2, o_depth2;       // byte offsets of the call's staged arrays in the workspace
    int has_depth;
    TriForm tf;
    TriPose pose;
};
struct TriCur { TriPose pose; float ratio_factor; int has_depth; };

// vt.row(3) of the SVD of the 4 x 4 float matrix whose COLUMNS are At[0..3] (At = A.t(), as cv::SVD::compute hands JacobiSVD the
// matrix).  Constant loop bounds and selects only: At, Vt and W stay in registers.
__device__ __forceinline__ void jacobi_vt3(float (&At)[4][4], float (&v)[4])
{
    float Vt[4][4];
    double W[4];
    const float eps = 1.1920928955078125e-7f * 2;       // FLT_EPSILON * 2
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float t = At[i][k]; sd += (double)t * t; Vt[i][k] = i == k ? 1.0f : 0.0f; }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) p += (double)At[i][k] * At[j][k];
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
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float t0 = c * At[i][k] + s * At[j][k];
                        const float t1 = -s * At[i][k] + c * At[j][k];
                        At[i][k] = t0; At[j][k] = t1;
                        a += (double)t0 * t0; b += (double)t1 * t1;
                        const float u0 = c * Vt[i][k] + s * Vt[j][k];
                        const float u1 = -s * Vt[i][k] + c * Vt[j][k];
                        Vt[i][k] = u0; Vt[j][k] = u1;
                    }
                    W[i] = a; W[j] = b;
                    changed = true;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    // the selection sort of the singular values (descending) applied to the row numbers: row[3] = where vt.row(3) comes from
    int row[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) { const bool m = wj < W[k]; j = m ? k : j; wj = m ? W[k] : wj; }
        const double wi = W[i];
        const int ri = row[i];
        int rj = ri;
#pragma unroll
        for (int k = i + 1; k < 4; ++k) {
            const bool m = j == k;
            rj = m ? row[k] : rj;
            W[k] = m ? wi : W[k];
            row[k] = m ? ri : row[k];
        }
        W[i] = wj; row[i] = rj;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = row[3] == 0 ? Vt[0][k] : row[3] == 1 ? Vt[1][k] : row[3] == 2 ? Vt[2][k] : Vt[3][k];
}

__device__ __forceinline__ double dot3d(const float *a, float b0, float b1, float b2)
{
    double s = 0;
    s += (double)a[0] * (double)b0; s += (double)a[1] * (double)b1; s += (double)a[2] * (double)b2;
    return s;
}

// One pair: the ORBM_TRI_* status, and x3D where the pair got as far as a point.
__device__ int triangulate_pair(const TriPose &c1, const TriPose &c2, const SeqKp &kp1, float depth1, const SeqKp &kp2, float depth2,
                                float ratioFactor, const float *__restrict__ scale, const float *__restrict__ sigma2, float (&x3D)[3])
{
    const bool bStereo1 = kp1.uright >= 0, bStereo2 = kp2.uright >= 0;                                     // :340, :344
    const float xn1x = (kp1.x - c1.cx) * c1.invfx, xn1y = (kp1.y - c1.cy) * c1.invfy;                      // :347-348
    const float xn2x = (kp2.x - c2.cx) * c2.invfx, xn2y = (kp2.y - c2.cy) * c2.invfy;
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { ray1[r] = gemm_row(c1.Rwc, r, xn1x, xn1y, 1.0f, 0.0f); ray2[r] = gemm_row(c2.Rwc, r, xn2x, xn2y, 1.0f, 0.0f); }
    const float cosParallaxRays = (float)(dot3d(ray1, ray2[0], ray2[1], ray2[2]) /
                                          (sqrt(dot3d(ray1, ray1[0], ray1[1], ray1[2])) * sqrt(dot3d(ray2, ray2[0], ray2[1], ray2[2]))));   // :352
    float cosParallaxStereo1 = cosParallaxRays + 1, cosParallaxStereo2 = cosParallaxRays + 1;
    if (bStereo1 || bStereo2) {                                                                            // :358-361
        float sn, cs;
        orbx_sincos_glibc_f32(2 * atan2f((bStereo1 ? c1.mb : c2.mb) / 2, bStereo1 ? depth1 : depth2), &sn, &cs);
        if (bStereo1) cosParallaxStereo1 = cs; else cosParallaxStereo2 = cs;
    }
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9997)) {   // :366
        float At[4][4], v[4];        // At[c][r] = A(r, c);  Tcw.row(r) = [Rcw(r, :) tcw(r)]
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float a0 = c < 3 ? c1.Rcw[c] : c1.tcw[0], a1 = c < 3 ? c1.Rcw[3 + c] : c1.tcw[1], a2 = c < 3 ? c1.Rcw[6 + c] : c1.tcw[2];
            const float b0 = c < 3 ? c2.Rcw[c] : c2.tcw[0], b1 = c < 3 ? c2.Rcw[3 + c] : c2.tcw[1], b2 = c < 3 ? c2.Rcw[6 + c] : c2.tcw[2];
            At[c][0] = xn1x * a2 + a0 * -1.0f; At[c][1] = xn1y * a2 + a1 * -1.0f;
            At[c][2] = xn2x * b2 + b0 * -1.0f; At[c][3] = xn2y * b2 + b1 * -1.0f;
        }
        jacobi_vt3(At, v);
        if (v[3] == 0) return ORBM_TRI_SVD_ZERO;                                                            // :380
        const float inv = (float)(1.0 / (double)v[3]);                                                     // :387
        x3D[0] = v[0] * inv; x3D[1] = v[1] * inv; x3D[2] = v[2] * inv;
    } else {
        const bool side1 = bStereo1 && cosParallaxStereo1 < cosParallaxStereo2;                            // :390-397
        const bool side2 = !side1 && bStereo2 && cosParallaxStereo2 < cosParallaxStereo1;
        if (!side1 && !side2) return ORBM_TRI_PARALLAX;
        const TriPose &c = side1 ? c1 : c2;                                                                // KeyFrame::UnprojectStereo, src/KeyFrame.cc:659-675
        const float z = side1 ? depth1 : depth2, u = side1 ? kp1.x : kp2.x, w = side1 ? kp1.y : kp2.y;
        if (!(z > 0)) return ORBM_TRI_PARALLAX;          // (the reference returns an empty Mat there and cannot go on)
        const float x = (u - c.cx) * z * c.invfx, y = (w - c.cy) * z * c.invfy;
#pragma unroll
        for (int r = 0; r < 3; ++r) x3D[r] = gemm_row(c.Rwc, r, x, y, z, c.Ow[r]);
    }
    const float z1 = (float)(dot3d(c1.Rcw + 6, x3D[0], x3D[1], x3D[2]) + (double)c1.tcw[2]);                 // :407
    if (z1 <= 0) return ORBM_TRI_DEPTH;
    const float z2 = (float)(dot3d(c2.Rcw + 6, x3D[0], x3D[1], x3D[2]) + (double)c2.tcw[2]);                 // :414
    if (z2 <= 0) return ORBM_TRI_DEPTH;
    {   // :421-452
        const float sigmaSquare1 = sigma2[kp1.octave];
        const float x1 = (float)(dot3d(c1.Rcw, x3D[0], x3D[1], x3D[2]) + (double)c1.tcw[0]);
        const float y1 = (float)(dot3d(c1.Rcw + 3, x3D[0], x3D[1], x3D[2]) + (double)c1.tcw[1]);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = c1.fx * x1 * invz1 + c1.cx, v1 = c1.fy * y1 * invz1 + c1.cy;
        const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y;
        if (!bStereo1) {
            if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) return ORBM_TRI_REPROJ1;
        } else {
            const float u1_r = u1 - c1.mbf * invz1, errX1_r = u1_r - kp1.uright;
            if ((double)(errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * (double)sigmaSquare1) return ORBM_TRI_REPROJ1;
        }
    }
    {   // :454-478; :471 takes the CURRENT keyframe's mbf
        const float sigmaSquare2 = sigma2[kp2.octave];
        const float x2 = (float)(dot3d(c2.Rcw, x3D[0], x3D[1], x3D[2]) + (double)c2.tcw[0]);
        const float y2 = (float)(dot3d(c2.Rcw + 3, x3D[0], x3D[1], x3D[2]) + (double)c2.tcw[1]);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = c2.fx * x2 * invz2 + c2.cx, v2 = c2.fy * y2 * invz2 + c2.cy;
        const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y;
        if (!bStereo2) {
            if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) return ORBM_TRI_REPROJ2;
        } else {
            const float u2_r = u2 - c1.mbf * invz2, errX2_r = u2_r - kp2.uright;
            if ((double)(errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * (double)sigmaSquare2) return ORBM_TRI_REPROJ2;
        }
    }
    // :480-497
    const float n10 = x3D[0] - c1.Ow[0], n11 = x3D[1] - c1.Ow[1], n12 = x3D[2] - c1.Ow[2];
    const float n20 = x3D[0] - c2.Ow[0], n21 = x3D[1] - c2.Ow[1], n22 = x3D[2] - c2.Ow[2];
    const float nn1[3] = {n10, n11, n12}, nn2[3] = {n20, n21, n22};
    const float dist1 = (float)sqrt(dot3d(nn1, n10, n11, n12)), dist2 = (float)sqrt(dot3d(nn2, n20, n21, n22));
    if (dist1 == 0 || dist2 == 0) return ORBM_TRI_DIST_ZERO;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = scale[kp1.octave] / scale[kp2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBM_TRI_SCALE;
    return ORBM_TRI_CREATED;
}

// CreateNewMapPoints' loop over the neighbours (:281-517) for every keypoint of the current keyframe at once: a 16-lane group per
// keypoint, in KF1's sorted order, walks the K neighbours in the caller's order -- the scan of k_triang_frames (only_stereo = 0),
// then lane 0 triangulates the winner and applies the gates.  What one neighbour leaves to the next is "the keypoint owns a point
// now" (ORBmatcher.cc:900-904), which is this group's own earlier result: kept in a register, no ordering between groups.
// Out, [K][n1] by feature index: match12 (-1 = none), status (ORBM_TRI_*), x3d where status = CREATED; counts[K][NSTATUS] += the
// tallies of statuses 0 .. 8 (zeroed by the caller).
constexpr int CP_MAX_K = 32;
__global__ __launch_bounds__(MT) void k_create_points(const SeqKp *__restrict__ kp1, const uint4 *__restrict__ A, const int *__restrict__ perm1,
                                                      int n1, TriCur cur, const TriNeigh *__restrict__ neigh, int K,
                                                      const char *__restrict__ arena, const uint8_t *__restrict__ hasmp1,
                                                      const float *__restrict__ depth1, const float *__restrict__ scale,
                                                      const float *__restrict__ sigma2, int *__restrict__ match12,
                                                      int8_t *__restrict__ status, float *__restrict__ x3d, int *__restrict__ counts)
{
    __shared__ int s_cnt[CP_MAX_K * ORBM_TRI_NSTATUS];
    for (int t = threadIdx.x; t < K * ORBM_TRI_NSTATUS; t += MT) s_cnt[t] = 0;
    __syncthreads();
    const int s = (blockIdx.x * MT + threadIdx.x) >> 4, sub = threadIdx.x & 15;
    if (s < n1) {                              // (whole 16-lane groups take the same way)
        const int i = perm1[s];
        const SeqKp k1 = kp1[s];
        const bool st1 = k1.uright >= 0;
        const uint4 a0 = A[2 * s], a1 = A[2 * s + 1];
        const float d1 = cur.has_depth ? depth1[i] : -1.0f;
        bool owned = hasmp1[i] != 0;
        for (int k = 0; k < K; ++k) {
            const TriNeigh &nb = neigh[k];
            int st = ORBM_TRI_SKIPPED, m = -1;
            float x3D[3] = {0.f, 0.f, 0.f};
            if (!owned) {                      // (uniform over the group)
                const int *cand = reinterpret_cast<const int *>(arena + nb.o_cand);
                const int k0 = reinterpret_cast<const int *>(arena + nb.o_cbeg)[i];
                const int kend = reinterpret_cast<const int *>(arena + nb.o_cend)[i];
                unsigned key = triang_scan(k1, st1, a0, a1, nb.tf, k0, kend, sub, cand,
                                           FrameKF2{nb.kp2, nb.perm2, reinterpret_cast<const uint8_t *>(arena + nb.o_has2)}, nb.B, scale, sigma2);
                key = orbx::row_min_u32(key);
                st = ORBM_TRI_NO_MATCH;
                if (key != 0xffffffffu) {
                    const int p = cand[k0 + (int)(0xffffu - (key & 0xffffu))];
                    m = nb.perm2[p];
                    if (sub == 0) {
                        const float d2 = nb.has_depth ? reinterpret_cast<const float *>(arena + nb.o_depth2)[m] : -1.0f;
                        st = triangulate_pair(cur.pose, nb.pose, k1, d1, nb.kp2[p], d2, cur.ratio_factor, scale, sigma2, x3D);
                    }
                    st = __shfl(st, 0, 16);
                    owned = st == ORBM_TRI_CREATED;
                }
            }
            if (sub == 0) {
                const size_t o = (size_t)k * n1 + i;
                match12[o] = m; status[o] = (int8_t)st;
                if (st == ORBM_TRI_CREATED) { x3d[3 * o] = x3D[0]; x3d[3 * o + 1] = x3D[1]; x3d[3 * o + 2] = x3D[2]; }
                if (st >= 0) atomicAdd(&s_cnt[k * ORBM_TRI_NSTATUS + st], 1);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K * ORBM_TRI_NSTATUS; t += MT)
        if (s_cnt[t]) atomicAdd(&counts[t], s_cnt[t]);
}

// The FeatureVector co-iteration of SearchForTriangulation (:881-891 / :1004-1012): every keypoint of a common node in KF1 scans
// the node's members of KF2, in member order -- the member lists once, as positions in KF2's arrays (cand[off2[nn2]]; inv2 =
// position of a feature index, nullptr: the index itself), and per keypoint of KF1 its list's bounds in cand (cbeg / cend [n1],
// zeroed by the caller).
int triang_candidates(const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1, const int32_t *nodes2,
                      const int32_t *off2, const int32_t *items2, int nn2, const int *inv2, int32_t *cbeg, int32_t *cend, int32_t *cand)
{
    const int nit2 = nn2 ? off2[nn2] : 0;
    for (int k = 0; k < nit2; ++k) cand[k] = inv2 ? inv2[items2[k]] : items2[k];
    bool fits = true;
    for_each_common_node(nodes1, nn1, nodes2, nn2, [&](int a, int b) {
        fits = fits && off2[b + 1] - off2[b] <= 65535;
        for (int k = off1[a]; k < off1[a + 1]; ++k) { cbeg[items1[k]] = off2[b]; cend[items1[k]] = off2[b + 1]; }
    });
    if (!fits) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 65,535 candidates for one keypoint (the tie rule's position field)");
    return ORBX_OK;
}

TriForm tri_form(const float *F12, float ex, float ey, int only_stereo)
{
    TriForm tf;
    for (int i = 0; i < 9; ++i) tf.F12[i] = F12[i];
    tf.ex = ex; tf.ey = ey; tf.only_stereo = only_stereo ? 1 : 0;
    return tf;
}

// The gated loop for the host-array entry points: keypoint i's candidates = cand[cbeg[i] .. cend[i]) of cand[nc], feature indices
// of KF2 (checked by the caller).  Out [n1]: match12, best_dist.
int triang_host_arrays(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbx_keypoint *kps2, const uint8_t *desc2, int n2,
                       const int32_t *cbeg, const int32_t *cend, const int32_t *cand, int nc, const uint8_t *has_mappoint1,
                       const uint8_t *has_mappoint2, const uint8_t *stereo1, const uint8_t *stereo2, int only_stereo, const float *F12,
                       float ex, float ey, const float *scale_factors2, const float *level_sigma2, int nlevels, int32_t *match12,
                       int32_t *best_dist)
{
    if ((n2 && !kps2) || (nc && (!desc2 || !has_mappoint2 || !stereo2))) ORBX_FAIL(ORBX_ERR_ARG, "bad candidate lists");
    for (int j = 0; j < n2; ++j)
        if (kps2[j].octave < 0 || kps2[j].octave >= nlevels) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    StagedCall sc;
    const size_t o_k1 = sc.in(kps1, sizeof(orbx_keypoint) * (size_t)n1), o_a = sc.in(desc1, (size_t)32 * n1),
                 o_k2 = sc.in(kps2, sizeof(orbx_keypoint) * (size_t)n2), o_b = sc.in(desc2, (size_t)32 * n2),
                 o_cb = sc.in(cbeg, sizeof(int) * (size_t)n1), o_ce = sc.in(cend, sizeof(int) * (size_t)n1),
                 o_ca = sc.in(cand, sizeof(int) * (size_t)nc), o_m1 = sc.in(has_mappoint1, (size_t)n1), o_m2 = sc.in(has_mappoint2, (size_t)n2),
                 o_s1 = sc.in(stereo1, (size_t)n1), o_s2 = sc.in(stereo2, (size_t)n2), o_sc = sc.in(scale_factors2, sizeof(float) * (size_t)nlevels),
                 o_sg = sc.in(level_sigma2, sizeof(float) * (size_t)nlevels), o_o = sc.out(sizeof(int) * 2 * (size_t)n1);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    int *ob = sc.d<int>(o_o);
    hipLaunchKernelGGL(k_triang_arrays, dim3((unsigned)(((size_t)n1 * 16 + MT - 1) / MT)), dim3(MT), 0, sc.stream(), sc.d<const orbx_keypoint>(o_k1),
                       sc.d<const uint4>(o_a), n1, sc.d<const orbx_keypoint>(o_k2), sc.d<const uint4>(o_b), sc.d<const int>(o_cb),
                       sc.d<const int>(o_ce), sc.d<const int>(o_ca), sc.d<const uint8_t>(o_m1), sc.d<const uint8_t>(o_m2), sc.d<const uint8_t>(o_s1),
                       sc.d<const uint8_t>(o_s2), tri_form(F12, ex, ey, only_stereo), sc.d<const float>(o_sc), sc.d<const float>(o_sg), ob, ob + n1);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(match12, sc.r<int>(o_o), sizeof(int) * (size_t)n1);
    memcpy(best_dist, sc.r<int>(o_o) + n1, sizeof(int) * (size_t)n1);
    return ORBX_OK;
}

std::atomic<int> g_last_create_points_waits{0};    // host waits of the last orbm_create_new_map_points call of this process

// What k_create_points needs of a keyframe's pose and camera: Rcw, tcw, Rwc = Rcw.t(), Ow = -Rwc * tcw (KeyFrame::SetPose).
void tri_pose(const orbm_triang_keyframe &kf, TriPose &p)
{
    pose_parts(kf.Tcw, p.Rcw, p.tcw);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p.Rwc[3 * c + r] = p.Rcw[3 * r + c];
    gemm3(p.Rwc, p.tcw, -1.0, nullptr, 0.0, p.Ow);
    p.fx = kf.fx; p.fy = kf.fy; p.cx = kf.cx; p.cy = kf.cy; p.invfx = kf.invfx; p.invfy = kf.invfy; p.mb = kf.mb; p.mbf = kf.mbf;
}

// The arguments of one keyframe of orbm_create_new_map_points; 0 = usable
int tri_check_keyframe(const orbm_triang_keyframe &kf, bool neighbour, int nlevels)
{
    if (!kf.frame || !kf.Tcw || kf.nn < 0 || (kf.nn && (!kf.nodes || !kf.off || !kf.items)) || (kf.frame->n && !kf.has_mappoint) ||
        (neighbour && !kf.F12))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (kf.frame->n > 8192) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in a keyframe");
    if (bow_check_items(kf.off, kf.items, kf.nn, kf.frame->n)) ORBX_FAIL(ORBX_ERR_ARG, "feature index out of range");
    if (kf.frame->n && (kf.frame->min_octave < 0 || kf.frame->max_octave >= nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    if (kf.frame->n && kf.frame->nstereo != 0 && !kf.depth) ORBX_FAIL(ORBX_ERR_ARG, "a frame with stereo keypoints needs its depths");
    return ORBX_OK;
}

} // namespace

extern "C" {

int orbm_frame_search_for_triangulation(const orbm_frame *kf1, const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1,
                                        const uint8_t *has_mappoint1, const orbm_frame *kf2, const int32_t *nodes2, const int32_t *off2,
                                        const int32_t *items2, int nn2, const uint8_t *has_mappoint2, int only_stereo, const float *F12,
                                        float ex, float ey, const float *scale_factors2, const float *level_sigma2, int nlevels,
                                        int check_orientation, int32_t *match12, int *nmatches)
{
    if (!kf1 || !kf2 || nn1 < 0 || nn2 < 0 || nlevels < 1 || !nmatches || !F12 || !scale_factors2 || !level_sigma2 ||
        (kf1->n && (!match12 || !has_mappoint1)) || (kf2->n && !has_mappoint2) || (nn1 && (!nodes1 || !off1 || !items1)) ||
        (nn2 && (!nodes2 || !off2 || !items2)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    const int n1 = kf1->n, n2 = kf2->n;
    if (bow_check_items(off1, items1, nn1, n1) || bow_check_items(off2, items2, nn2, n2)) ORBX_FAIL(ORBX_ERR_ARG, "feature index out of range");
    if (n2 && (kf2->min_octave < 0 || kf2->max_octave >= nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    *nmatches = 0;
    if (n1 == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    std::vector<int32_t> cbeg((size_t)n1, 0), cend((size_t)n1, 0), cand((size_t)std::max(nn2 ? off2[nn2] : 0, 1));
    {
        const int rc = triang_candidates(nodes1, off1, items1, nn1, nodes2, off2, items2, nn2, kf2->inv_host.data(), cbeg.data(), cend.data(),
                                         cand.data());
        if (rc != ORBX_OK) return rc;
    }
    StagedCall sc;
    const size_t o_cb = sc.in(cbeg.data(), sizeof(int) * (size_t)n1), o_ce = sc.in(cend.data(), sizeof(int) * (size_t)n1),
                 o_ca = sc.in(cand.data(), sizeof(int) * cand.size()), o_m1 = sc.in(has_mappoint1, (size_t)n1),
                 o_m2 = sc.in(has_mappoint2, (size_t)n2), o_sc = sc.in(scale_factors2, sizeof(float) * (size_t)nlevels),
                 o_sg = sc.in(level_sigma2, sizeof(float) * (size_t)nlevels), o_o = sc.out(sizeof(int) * 2 * (size_t)n1);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    int *om = sc.d<int>(o_o);
    hipLaunchKernelGGL(k_triang_frames, dim3((unsigned)(((size_t)n1 * 16 + MT - 1) / MT)), dim3(MT), 0, sc.stream(), (const SeqKp *)kf1->kp,
                       (const uint4 *)kf1->desc, (const float *)kf1->angle, (const int *)kf1->perm, n1, (const SeqKp *)kf2->kp,
                       (const uint4 *)kf2->desc, (const float *)kf2->angle, (const int *)kf2->perm, sc.d<const int>(o_cb),
                       sc.d<const int>(o_ce), sc.d<const int>(o_ca), sc.d<const uint8_t>(o_m1), sc.d<const uint8_t>(o_m2),
                       tri_form(F12, ex, ey, only_stereo), sc.d<const float>(o_sc), sc.d<const float>(o_sg), om, reinterpret_cast<float *>(om + n1));
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(match12, sc.r<int>(o_o), sizeof(int) * (size_t)n1);
    const float *rot = reinterpret_cast<const float *>(sc.r<int>(o_o) + n1);      // angle1 - angle2 of every pair (:994)
    return triangulation_rotation_check(match12, n1, check_orientation, [&](int i) { return rot[i]; }, nmatches);
}

int orbm_match_triangulation(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbx_keypoint *kps2,
                             const uint8_t *desc2, int n2, const int32_t *cand_off, const int32_t *cand_idx,
                             const uint8_t *has_mappoint1, const uint8_t *has_mappoint2, const uint8_t *stereo1,
                             const uint8_t *stereo2, int only_stereo, const float *F12, float ex, float ey,
                             const float *scale_factors2, const float *level_sigma2, int nlevels, int32_t *match12,
                             int32_t *best_dist)
{
    if (n1 < 0 || n2 < 0 || nlevels < 1 || (n1 && (!kps1 || !desc1 || !has_mappoint1 || !stereo1 || !match12 || !best_dist)) ||
        !cand_off || !F12 || !scale_factors2 || !level_sigma2)
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    if (n1 == 0) return ORBX_OK;
    const int nc = cand_off[n1];
    if (nc < 0 || (nc && !cand_idx)) ORBX_FAIL(ORBX_ERR_ARG, "bad candidate lists");
    for (int k = 0; k < nc; ++k)
        if (cand_idx[k] < 0 || cand_idx[k] >= n2) ORBX_FAIL(ORBX_ERR_ARG, "candidate index out of range");
    for (int i = 0; i < n1; ++i)
        if (cand_off[i] > cand_off[i + 1] || cand_off[i] < 0) ORBX_FAIL(ORBX_ERR_ARG, "candidate offsets not monotone");
    for (int i = 0; i < n1; ++i)
        if (cand_off[i + 1] - cand_off[i] > 65535) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 65,535 candidates for one keypoint (the tie rule's position field)");
    return triang_host_arrays(kps1, desc1, n1, kps2, desc2, n2, cand_off, cand_off + 1, cand_idx, nc, has_mappoint1, has_mappoint2, stereo1,
                              stereo2, only_stereo, F12, ex, ey, scale_factors2, level_sigma2, nlevels, match12, best_dist);
}

// The whole ORBmatcher::SearchForTriangulation (ORBmatcher.cc:858-1024) in one call: the FeatureVector co-iteration
// (triang_candidates), the gated loop on the device, the rotation histogram, ComputeThreeMaxima and the rejection (:992-1012).  A
// FeatureVector = (nodes ascending, off, items), as for orbm_search_by_bow.  match12[n1] = index in KF2 or -1; the pair list
// vMatchedPairs is its non-negative entries in index order (:1014-1021).
int orbm_search_for_triangulation(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const int32_t *nodes1, const int32_t *off1,
                                  const int32_t *items1, int nn1, const uint8_t *has_mappoint1, const uint8_t *stereo1,
                                  const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const int32_t *nodes2, const int32_t *off2,
                                  const int32_t *items2, int nn2, const uint8_t *has_mappoint2, const uint8_t *stereo2, int only_stereo,
                                  const float *F12, float ex, float ey, const float *scale_factors2, const float *level_sigma2, int nlevels,
                                  int check_orientation, int32_t *match12, int *nmatches)
{
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || !nmatches || (n1 && !match12) || (nn1 && (!nodes1 || !off1 || !items1)) ||
        (nn2 && (!nodes2 || !off2 || !items2)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    *nmatches = 0;
    if (n1 == 0) return ORBX_OK;
    if (bow_check_items(off1, items1, nn1, n1) || bow_check_items(off2, items2, nn2, n2)) ORBX_FAIL(ORBX_ERR_ARG, "feature index out of range");
    if (nlevels < 1 || !kps1 || !desc1 || !has_mappoint1 || !stereo1 || !F12 || !scale_factors2 || !level_sigma2)
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    const int nc = nn2 ? off2[nn2] : 0;
    std::vector<int32_t> cbeg((size_t)n1, 0), cend((size_t)n1, 0), cand((size_t)std::max(nc, 1)), best((size_t)n1);
    int rc = triang_candidates(nodes1, off1, items1, nn1, nodes2, off2, items2, nn2, nullptr, cbeg.data(), cend.data(), cand.data());
    if (rc == ORBX_OK)
        rc = triang_host_arrays(kps1, desc1, n1, kps2, desc2, n2, cbeg.data(), cend.data(), cand.data(), nc, has_mappoint1, has_mappoint2, stereo1,
                                stereo2, only_stereo, F12, ex, ey, scale_factors2, level_sigma2, nlevels, match12, best.data());
    if (rc != ORBX_OK) return rc;
    return triangulation_rotation_check(match12, n1, check_orientation,
                                        [&](int i) { return kps1[i].angle - kps2[match12[i]].angle; }, nmatches);     // :994
}

// LocalMapping::CreateNewMapPoints' loop over the neighbour keyframes (src/LocalMapping.cc:281-517) in one launch: see k_create_points.
int orbm_create_new_map_points(const orbm_triang_keyframe *cur, const orbm_triang_keyframe *neigh, int K, const float *scale_factors,
                               const float *level_sigma2, int nlevels, float scale_factor, int32_t *match12, int8_t *status, float *x3d,
                               int32_t *counts, int *nnew)
{
    g_last_create_points_waits.store(0, std::memory_order_relaxed);
    if (K < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (K > CP_MAX_K) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 32 neighbour keyframes in one call");
    if (!cur || (K && !neigh) || !scale_factors || !level_sigma2 || nlevels < 1 || !nnew) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    int rc = tri_check_keyframe(*cur, false, nlevels);
    for (int k = 0; k < K && rc == ORBX_OK; ++k) rc = tri_check_keyframe(neigh[k], true, nlevels);
    if (rc != ORBX_OK) return rc;
    const int n1 = cur->frame->n;
    if (n1 && K && (!match12 || !status || !x3d)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    *nnew = 0;
    if (counts) memset(counts, 0, sizeof(int32_t) * (size_t)K * ORBM_TRI_NSTATUS);
    if (K == 0 || n1 == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    // per neighbour: the candidate lists of the co-iteration, its mask and depths, staged behind each other
    std::vector<TriNeigh> nb((size_t)K);
    std::vector<std::vector<int32_t>> cbeg((size_t)K), cend((size_t)K), cand((size_t)K);
    StagedCall sc;
    const size_t o_m1 = sc.in(cur->has_mappoint, (size_t)n1), o_d1 = sc.in(cur->depth, sizeof(float) * (size_t)n1),
                 o_sc = sc.in(scale_factors, sizeof(float) * (size_t)nlevels), o_sg = sc.in(level_sigma2, sizeof(float) * (size_t)nlevels);
    for (int k = 0; k < K; ++k) {
        const orbm_triang_keyframe &kf = neigh[k];
        const int n2 = kf.frame->n;
        cbeg[k].assign((size_t)n1, 0); cend[k].assign((size_t)n1, 0); cand[k].assign((size_t)std::max(kf.nn ? kf.off[kf.nn] : 0, 1), 0);
        rc = triang_candidates(cur->nodes, cur->off, cur->items, cur->nn, kf.nodes, kf.off, kf.items, kf.nn, kf.frame->inv_host.data(),
                               cbeg[k].data(), cend[k].data(), cand[k].data());
        if (rc != ORBX_OK) return rc;
        TriNeigh &t = nb[k];
        t.kp2 = kf.frame->kp; t.B = kf.frame->desc; t.perm2 = kf.frame->perm;
        t.o_cbeg = (unsigned)sc.in(cbeg[k].data(), sizeof(int) * (size_t)n1);
        t.o_cend = (unsigned)sc.in(cend[k].data(), sizeof(int) * (size_t)n1);
        t.o_cand = (unsigned)sc.in(cand[k].data(), sizeof(int) * cand[k].size());
        t.o_has2 = (unsigned)sc.in(kf.has_mappoint, (size_t)n2);
        t.o_depth2 = (unsigned)sc.in(kf.depth, sizeof(float) * (size_t)n2);
        t.has_depth = kf.depth ? 1 : 0;
        t.tf = tri_form(kf.F12, kf.ex, kf.ey, 0);                                     // SearchForTriangulation(.., false), :315
        tri_pose(kf, t.pose);
    }
    const size_t o_nb = sc.in(nb.data(), sizeof(TriNeigh) * (size_t)K);
    const size_t kn = (size_t)K * (size_t)n1;
    const size_t o_m = sc.out(sizeof(int) * kn), o_x = sc.out(sizeof(float) * 3 * kn), o_c = sc.out(sizeof(int) * (size_t)K * ORBM_TRI_NSTATUS),
                 o_s = sc.out(kn);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    TriCur tc;
    tri_pose(*cur, tc.pose);
    tc.ratio_factor = 1.5f * scale_factor;                                             // :276
    tc.has_depth = cur->depth ? 1 : 0;
    ORBX_HIP(hipMemsetAsync(sc.d<int>(o_c), 0, sizeof(int) * (size_t)K * ORBM_TRI_NSTATUS, sc.stream()));
    hipLaunchKernelGGL(k_create_points, dim3((unsigned)(((size_t)n1 * 16 + MT - 1) / MT)), dim3(MT), 0, sc.stream(),
                       (const SeqKp *)cur->frame->kp, (const uint4 *)cur->frame->desc, (const int *)cur->frame->perm, n1, tc,
                       sc.d<const TriNeigh>(o_nb), K, sc.d<const char>(0), sc.d<const uint8_t>(o_m1), sc.d<const float>(o_d1),
                       sc.d<const float>(o_sc), sc.d<const float>(o_sg), sc.d<int>(o_m), sc.d<int8_t>(o_s), sc.d<float>(o_x), sc.d<int>(o_c));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_create_points_waits.store(sc.waits, std::memory_order_relaxed);     // counted where the stream is waited for
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(match12, sc.r<int>(o_m), sizeof(int) * kn);
    memcpy(status, sc.r<int8_t>(o_s), kn);
    if (counts) memcpy(counts, sc.r<int>(o_c), sizeof(int) * (size_t)K * ORBM_TRI_NSTATUS);
    const float *rx = sc.r<float>(o_x);
    int created = 0;
    for (size_t o = 0; o < kn; ++o)
        if (status[o] == ORBM_TRI_CREATED) { memcpy(x3d + 3 * o, rx + 3 * o, sizeof(float) * 3); ++created; }
    *nnew = created;
    return ORBX_OK;
}

int orbm_debug_last_create_points_waits(void) { return g_last_create_points_waits.load(std::memory_order_relaxed); }

} // extern "C"
