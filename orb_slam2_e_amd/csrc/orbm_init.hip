// orbm_init.hip -- the monocular Initializer (src/Initializer.cc) on the device.
//
// Initialize (:44-121) draws the 8-point sets of all iterations before the first one runs (:77-97); no hypothesis reads another's
// result, and what FindHomography / FindFundamental return is a fold over per-hypothesis scores.  So:
//   orbm_init_find_models     k_init_models: one wave per (model, hypothesis), 2 H waves in ONE launch.  H side: ComputeH21
//                             (:226-266), H21i = T2inv Hn T1, H12i = H21i.inv(), CheckHomography (:305-388).  F side: ComputeF21
//                             (:268-303), F21i = T2t Fn T1, CheckFundamental (:390-468).  Every lane computes the model from the
//                             same inputs (the same bits in every lane: no broadcast, no barrier), then the lanes take a match
//                             each, 64 per round.  The score is the reference's SEQUENTIAL float sum: the lanes compute their two
//                             terms, and the wave adds the 128 terms of a round in match order with readlanes into one
//                             accumulator.  __ballot words are the inlier mask.  Normalize (:749-795), T2.inv(), T2.t() and the
//                             fold (:148-171, :199-222) run on the host.
//   orbm_init_check_rt        k_init_check_rt: CheckRT (:798-907) of up to 8 motions, a thread per (motion, match): Triangulate
//                             (:734-747) with the 4 x 4 SVD, the finiteness test, cosParallax, both depth tests, both
//                             reprojection tests.  P1, P2, O2 per motion, the scatter into vbGood / vP3D in match order, the sort
//                             of the counted cosines and acosf run on the host.
//   orbm_init_reconstruct_f   ReconstructF (:470-570): E21, DecomposeE (:909-929) and the choice among the four motions on the
//                             host, around one orbm_init_check_rt call.
// Each call: one staged upload, one launch, one host wait, on a leased workspace.  The arithmetic is the reference's float / double
// order op by op with OpenCV 3.4's cv::Mat semantics (orbm_svd.h; unpinned like every OpenCV primitive here).  No
// float atomics; every sum has a fixed order; -ffp-contract=off.  ReconstructH (:572-732) is not here.
#include <algorithm>
#include <atomic>

#include "orbm_internal.h"
#include "orbm_svd.h"

using namespace orbm_detail;

namespace {

constexpr int INIT_MAX_N = 8192, INIT_MAX_H = 1024, INIT_MAX_M = 8;

struct InitDev {
    float T1[9], T2inv[9], T2t[9];
    float inv_sigma2;
    int n, H;
    unsigned o_pts, o_npts, o_sets;      // staged: [n] float4 (u1, v1, u2, v2) in pixels; the same normalised; [H][8] ints
    unsigned o_mat, o_score, o_mask;     // results: [2 H][9], [2 H], [2 H][(n + 63) / 64]; the H model first
};

__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(64) void k_init_models(InitDev d, char *__restrict__ ws)
{
    const int lane = threadIdx.x;
    const int g = blockIdx.x;                                           // the wave's (model, hypothesis): the same in every lane
    const bool fundamental = g >= d.H;
    const int h = fundamental ? g - d.H : g;
    const float4 *npts = reinterpret_cast<const float4 *>(ws + d.o_npts);
    const int *set = reinterpret_cast<const int *>(ws + d.o_sets) + 8 * h;
    float m[9], minv[9];                                                // H21i and H12i, or F21i
    if (!fundamental) {
        float At[9][16], v[9], tmp[9];                                  // At[c][r] = A(r, c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 p = npts[set[j]];                              // inside [0, n): checked on the host before the launch
            const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
            At[0][2 * j] = 0.0f; At[1][2 * j] = 0.0f; At[2][2 * j] = 0.0f;
            At[3][2 * j] = -u1; At[4][2 * j] = -v1; At[5][2 * j] = -1.0f;
            At[6][2 * j] = v2 * u1; At[7][2 * j] = v2 * v1; At[8][2 * j] = v2;
            At[0][2 * j + 1] = u1; At[1][2 * j + 1] = v1; At[2][2 * j + 1] = 1.0f;
            At[3][2 * j + 1] = 0.0f; At[4][2 * j + 1] = 0.0f; At[5][2 * j + 1] = 0.0f;
            At[6][2 * j + 1] = -u2 * u1; At[7][2 * j + 1] = -u2 * v1; At[8][2 * j + 1] = -u2;
        }
        orbm_svd::svd_16x9_vt8(At, v);
        orbm_svd::gemm33(d.T2inv, v, tmp);
        orbm_svd::gemm33(tmp, d.T1, m);
        orbm_svd::invert33(m, minv);
    } else {
        float At[9][9], v[9], w[3], u[9], vt[9], tmp[9], fn[9];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 p = npts[set[j]];
            const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
            At[j][0] = u2 * u1; At[j][1] = u2 * v1; At[j][2] = u2;
            At[j][3] = v2 * u1; At[j][4] = v2 * v1; At[j][5] = v2;
            At[j][6] = u1; At[j][7] = v1; At[j][8] = 1.0f;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) At[8][k] = 0.0f;
        orbm_svd::svd_8x9_vt8(At, v);
        orbm_svd::svd33(v, w, u, vt);
        w[2] = 0.0f;
        const float dg[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, w[2]};    // cv::Mat::diag(w)
        orbm_svd::gemm33(u, dg, tmp);
        orbm_svd::gemm33(tmp, vt, fn);
        orbm_svd::gemm33(d.T2t, fn, tmp);
        orbm_svd::gemm33(tmp, d.T1, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) minv[k] = 0.0f;
    }
    if (lane == 0) {
        float *o = reinterpret_cast<float *>(ws + d.o_mat) + 9 * g;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = m[k];
    }
    const float4 *pts = reinterpret_cast<const float4 *>(ws + d.o_pts);
    const int n = d.n, words = (n + 63) >> 6;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(ws + d.o_mask) + (size_t)g * words;
    const float inv_sigma2 = d.inv_sigma2;
    float score = 0;
    for (int w = 0; w < words; ++w) {
        const int i = 64 * w + lane;
        float term1 = 0.0f, term2 = 0.0f;                               // what the match adds to the score; adding +0 changes no bit
        bool in = false;
        if (i < n) {
            const float4 p = pts[i];
            const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
            float chi1, chi2, th, th_score;
            if (!fundamental) {                                         // CheckHomography :344-379
                th = 5.991f; th_score = 5.991f;
                const float w2in1inv = (float)(1.0 / (double)(minv[6] * u2 + minv[7] * v2 + minv[8]));
                const float u2in1 = (minv[0] * u2 + minv[1] * v2 + minv[2]) * w2in1inv;
                const float v2in1 = (minv[3] * u2 + minv[4] * v2 + minv[5]) * w2in1inv;
                const float sd1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
                chi1 = sd1 * inv_sigma2;
                const float w1in2inv = (float)(1.0 / (double)(m[6] * u1 + m[7] * v1 + m[8]));
                const float u1in2 = (m[0] * u1 + m[1] * v1 + m[2]) * w1in2inv;
                const float v1in2 = (m[3] * u1 + m[4] * v1 + m[5]) * w1in2inv;
                const float sd2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
                chi2 = sd2 * inv_sigma2;
            } else {                                                    // CheckFundamental :420-459
                th = 3.841f; th_score = 5.991f;
                const float a2 = m[0] * u1 + m[1] * v1 + m[2];
                const float b2 = m[3] * u1 + m[4] * v1 + m[5];
                const float c2 = m[6] * u1 + m[7] * v1 + m[8];
                const float num2 = a2 * u2 + b2 * v2 + c2;
                const float sd1 = num2 * num2 / (a2 * a2 + b2 * b2);
                chi1 = sd1 * inv_sigma2;
                const float a1 = m[0] * u2 + m[3] * v2 + m[6];
                const float b1 = m[1] * u2 + m[4] * v2 + m[7];
                const float c1 = m[2] * u2 + m[5] * v2 + m[8];
                const float num1 = a1 * u1 + b1 * v1 + c1;
                const float sd2 = num1 * num1 / (a1 * a1 + b1 * b1);
                chi2 = sd2 * inv_sigma2;
            }
            in = true;                                                  // a NaN chiSquare is not > th: it stays in and makes the score NaN
            if (chi1 > th) in = false; else term1 = th_score - chi1;
            if (chi2 > th) in = false; else term2 = th_score - chi2;
        }
        const unsigned long long word = __ballot(in);                   // bits past n are 0
        if (lane == 0) mask[w] = word;
        // score += term1; score += term2; for the matches 64 w .. 64 w + 63 in this order, the same in every lane
#pragma unroll
        for (int l = 0; l < 64; ++l) {
            score += lane_value(term1, l);
            score += lane_value(term2, l);
        }
    }
    if (lane == 0) reinterpret_cast<float *>(ws + d.o_score)[g] = score;
}

// ------------------------------------------------------------------------------------------------ CheckRT
struct RtMotion { float R[9], t[3], P2[12], O2[3]; };
struct RtDev {
    float P1[12], fx, fy, cx, cy, th2;
    int n, M;
    unsigned o_pts, o_inl, o_mot;        // staged: [n] float4, [n] bytes, [M] RtMotion
    unsigned o_state, o_cos, o_p3d;      // results per (motion, match): RT_* byte, cosParallax, p3dC1
};
enum { RT_NONE = 0, RT_NOT_FINITE = 1, RT_COUNTED = 2, RT_GOOD = 3 };

__global__ __launch_bounds__(MT) void k_init_check_rt(RtDev d, char *__restrict__ ws)
{
    const int i = blockIdx.x * MT + threadIdx.x, mi = blockIdx.y;
    if (i >= d.n) return;
    const size_t o = (size_t)mi * d.n + i;
    uint8_t *state = reinterpret_cast<uint8_t *>(ws + d.o_state) + o;
    float *cosp = reinterpret_cast<float *>(ws + d.o_cos) + o, *p3d = reinterpret_cast<float *>(ws + d.o_p3d) + 3 * o;
    int st = RT_NONE;
    float cos_out = 0.0f, x[3] = {0.0f, 0.0f, 0.0f};
    if (reinterpret_cast<const uint8_t *>(ws + d.o_inl)[i]) {
        const RtMotion &mo = reinterpret_cast<const RtMotion *>(ws + d.o_mot)[mi];
        const float4 p = reinterpret_cast<const float4 *>(ws + d.o_pts)[i];
        float At[4][4], v[4];                                           // Triangulate :734-747; At[c][r] = A(r, c)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            At[c][0] = p.x * d.P1[8 + c] + d.P1[c] * -1.0f; At[c][1] = p.y * d.P1[8 + c] + d.P1[4 + c] * -1.0f;
            At[c][2] = p.z * mo.P2[8 + c] + mo.P2[c] * -1.0f; At[c][3] = p.w * mo.P2[8 + c] + mo.P2[4 + c] * -1.0f;
        }
        orbm_svd::svd_4x4_vt3(At, v);
        const float inv = (float)(1.0 / (double)v[3]);
        const float X = v[0] * inv, Y = v[1] * inv, Z = v[2] * inv;
        if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) st = RT_NOT_FINITE;
        else {
            const float n1[3] = {X - 0.0f, Y - 0.0f, Z - 0.0f}, n2[3] = {X - mo.O2[0], Y - mo.O2[1], Z - mo.O2[2]};
            double s1 = 0, s2 = 0, dt = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { s1 += (double)n1[k] * n1[k]; s2 += (double)n2[k] * n2[k]; dt += (double)n1[k] * n2[k]; }
            const float dist1 = (float)sqrt(s1), dist2 = (float)sqrt(s2);
            const float cosParallax = (float)(dt / (double)(dist1 * dist2));
            const bool low = (double)cosParallax < 0.9998;
            bool go = !(Z <= 0 && low);
            float X2 = 0, Y2 = 0, Z2 = 0;
            if (go) {
                X2 = gemm_row(mo.R, 0, X, Y, Z, mo.t[0]); Y2 = gemm_row(mo.R, 1, X, Y, Z, mo.t[1]); Z2 = gemm_row(mo.R, 2, X, Y, Z, mo.t[2]);
                go = !(Z2 <= 0 && low);
            }
            if (go) {
                const float invZ1 = (float)(1.0 / (double)Z);
                const float im1x = d.fx * X * invZ1 + d.cx, im1y = d.fy * Y * invZ1 + d.cy;
                const float e1 = (im1x - p.x) * (im1x - p.x) + (im1y - p.y) * (im1y - p.y);
                go = !(e1 > d.th2);
            }
            if (go) {
                const float invZ2 = (float)(1.0 / (double)Z2);
                const float im2x = d.fx * X2 * invZ2 + d.cx, im2y = d.fy * Y2 * invZ2 + d.cy;
                const float e2 = (im2x - p.z) * (im2x - p.z) + (im2y - p.w) * (im2y - p.w);
                go = !(e2 > d.th2);
            }
            if (go) {
                st = low ? RT_GOOD : RT_COUNTED;
                cos_out = cosParallax; x[0] = X; x[1] = Y; x[2] = Z;
            }
        }
    }
    *state = (uint8_t)st; *cosp = cos_out;
    p3d[0] = x[0]; p3d[1] = x[1]; p3d[2] = x[2];
}

std::atomic<int> g_last_init_waits{0};     // host waits of the last orbm_init_* call of this process

// Normalize (:749-795): all keypoints of the frame, sequential float sums
void normalize(const float *keys, int N, std::vector<float> &pn, float *T)
{
    float meanX = 0, meanY = 0;
    pn.resize((size_t)2 * N);
    for (int i = 0; i < N; ++i) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; ++i) {
        pn[2 * i] = keys[2 * i] - meanX; pn[2 * i + 1] = keys[2 * i + 1] - meanY;
        meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
    }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    const float sX = (float)(1.0 / meanDevX), sY = (float)(1.0 / meanDevY);
    for (int i = 0; i < N; ++i) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    for (int k = 0; k < 9; ++k) T[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    T[0] = sX; T[4] = sY; T[2] = -meanX * sX; T[5] = -meanY * sY;
}

// the arguments every call shares: 0, or the refusal
int check_matches(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n)
{
    if (n < 0 || n1 < 0 || n2 < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > INIT_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 matches");
    if (n && (!keys1 || !keys2 || !matches)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    for (int i = 0; i < n; ++i)
        if (matches[2 * i] < 0 || matches[2 * i] >= n1 || matches[2 * i + 1] < 0 || matches[2 * i + 1] >= n2)
            ORBX_FAIL(ORBX_ERR_ARG, "match index outside its frame");
    return ORBX_OK;
}

void gather(const float *k1, const float *k2, const int32_t *matches, int n, std::vector<float> &pts)
{
    pts.resize((size_t)4 * std::max(n, 1));
    for (int i = 0; i < n; ++i) {
        const int a = matches[2 * i], b = matches[2 * i + 1];
        pts[4 * i] = k1[2 * a]; pts[4 * i + 1] = k1[2 * a + 1]; pts[4 * i + 2] = k2[2 * b]; pts[4 * i + 3] = k2[2 * b + 1];
    }
}

// the 3 x 4 product K * [R | t] (gemm's small-matrix case: float row sums)
void k_times_rt(const float *K, const float *R, const float *t, float *P)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            const float s = K[3 * r] * b0 + K[3 * r + 1] * b1 + K[3 * r + 2] * b2;
            P[4 * r + c] = (float)((double)s * 1.0 + (double)0.0f * 0.0);
        }
}

} // namespace

extern "C" {

int orbm_init_find_models(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n, const int32_t *sets, int H,
                          float sigma, orbm_init_models *out, void *mask_h, void *mask_f, float *hyp_matrices, float *hyp_scores,
                          void *hyp_masks)
{
    g_last_init_waits.store(0, std::memory_order_relaxed);
    if (H < 0 || !out) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (!(sigma > 0)) ORBX_FAIL(ORBX_ERR_ARG, "sigma must be positive");
    if (H > INIT_MAX_H) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,024 hypotheses");
    if (const int rc = check_matches(keys1, n1, keys2, n2, matches, n)) return rc;
    if (H > 0 && n < 8) ORBX_FAIL(ORBX_ERR_ARG, "a hypothesis needs eight matches");
    if (H > 0 && (!sets || !mask_h || !mask_f)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    for (int h = 0; h < H; ++h)
        for (int j = 0; j < 8; ++j) {
            const int32_t a = sets[8 * h + j];
            if (a < 0 || a >= n) ORBX_FAIL(ORBX_ERR_ARG, "set index out of range");
            for (int k = 0; k < j; ++k)
                if (sets[8 * h + k] == a) ORBX_FAIL(ORBX_ERR_ARG, "a set repeats an index");
        }
    const size_t words = (size_t)((n + 63) / 64);
    memset(out, 0, sizeof(*out));
    out->itH = -1; out->itF = -1;
    if (mask_h) memset(mask_h, 0, sizeof(uint64_t) * words);
    if (mask_f) memset(mask_f, 0, sizeof(uint64_t) * words);
    if (H == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    InitDev d;
    memset(&d, 0, sizeof(d));
    std::vector<float> pn1, pn2, pts, npts;
    float T2[9];
    normalize(keys1, n1, pn1, d.T1);
    normalize(keys2, n2, pn2, T2);
    orbm_svd::invert33(T2, d.T2inv);
    transpose3(T2, d.T2t);
    gather(keys1, keys2, matches, n, pts);
    gather(pn1.data(), pn2.data(), matches, n, npts);
    d.inv_sigma2 = (float)(1.0 / (sigma * sigma));
    d.n = n; d.H = H;
    StagedCall sc;
    d.o_pts = (unsigned)sc.in(pts.data(), sizeof(float) * 4 * (size_t)n);
    d.o_npts = (unsigned)sc.in(npts.data(), sizeof(float) * 4 * (size_t)n);
    d.o_sets = (unsigned)sc.in(sets, sizeof(int32_t) * 8 * (size_t)H);
    d.o_mat = (unsigned)sc.out(sizeof(float) * 9 * 2 * (size_t)H);
    d.o_score = (unsigned)sc.out(sizeof(float) * 2 * (size_t)H);
    d.o_mask = (unsigned)sc.out(sizeof(uint64_t) * 2 * (size_t)H * words);
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_init_models, dim3((unsigned)(2 * H)), dim3(64), 0, sc.stream(), d, sc.d<char>(0));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_init_waits.store(sc.waits, std::memory_order_relaxed);
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    const float *mat = sc.r<float>(d.o_mat), *score = sc.r<float>(d.o_score);
    const uint64_t *mask = sc.r<uint64_t>(d.o_mask);
    if (hyp_matrices) memcpy(hyp_matrices, mat, sizeof(float) * 9 * 2 * (size_t)H);
    if (hyp_scores) memcpy(hyp_scores, score, sizeof(float) * 2 * (size_t)H);
    if (hyp_masks) memcpy(hyp_masks, mask, sizeof(uint64_t) * 2 * (size_t)H * words);
    // the folds of :148-171 and :199-222: the first hypothesis whose score is > every earlier one, starting from 0 (a NaN and a 0
    // never win)
    for (int model = 0; model < 2; ++model) {
        float best = 0.0f;
        int it = -1;
        for (int h = 0; h < H; ++h)
            if (score[model * H + h] > best) { best = score[model * H + h]; it = h; }
        if (it >= 0) {
            memcpy(model ? out->F21 : out->H21, mat + 9 * (size_t)(model * H + it), sizeof(float) * 9);
            memcpy(model ? mask_f : mask_h, mask + (size_t)(model * H + it) * words, sizeof(uint64_t) * words);
        }
        if (model) { out->SF = best; out->itF = it; } else { out->SH = best; out->itH = it; }
    }
    return ORBX_OK;
}

int orbm_init_check_rt(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n, const uint8_t *inliers,
                       const float *K, const float *R, const float *t, int M, float th2, uint8_t *good, float *P3D, uint8_t *counted,
                       float *cos_parallax, int32_t *ngood, float *parallax)
{
    g_last_init_waits.store(0, std::memory_order_relaxed);
    if (M < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (M > INIT_MAX_M) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8 motions");
    if (const int rc = check_matches(keys1, n1, keys2, n2, matches, n)) return rc;
    if (M == 0) return ORBX_OK;
    if (!K || !R || !t || !good || !P3D || !ngood || !parallax || (n && !inliers)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    memset(good, 0, (size_t)M * (size_t)n1);
    memset(P3D, 0, sizeof(float) * 3 * (size_t)M * (size_t)n1);
    if (counted) memset(counted, 0, (size_t)M * (size_t)n);
    if (cos_parallax) memset(cos_parallax, 0, sizeof(float) * (size_t)M * (size_t)n);
    for (int m = 0; m < M; ++m) { ngood[m] = 0; parallax[m] = 0.0f; }
    if (n == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    RtDev d;
    memset(&d, 0, sizeof(d));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) d.P1[4 * r + c] = c < 3 ? K[3 * r + c] : 0.0f;       // K.copyTo into a zero 3 x 4
    d.fx = K[0]; d.fy = K[4]; d.cx = K[2]; d.cy = K[5]; d.th2 = th2; d.n = n; d.M = M;
    std::vector<RtMotion> mot((size_t)M);
    for (int m = 0; m < M; ++m) {
        RtMotion &q = mot[m];
        memcpy(q.R, R + 9 * m, sizeof(q.R)); memcpy(q.t, t + 3 * m, sizeof(q.t));
        k_times_rt(K, q.R, q.t, q.P2);
        neg_Rt_t(q.R, q.t, q.O2);
    }
    std::vector<float> pts;
    gather(keys1, keys2, matches, n, pts);
    const size_t mn = (size_t)M * (size_t)n;
    StagedCall sc;
    d.o_pts = (unsigned)sc.in(pts.data(), sizeof(float) * 4 * (size_t)n);
    d.o_inl = (unsigned)sc.in(inliers, (size_t)n);
    d.o_mot = (unsigned)sc.in(mot.data(), sizeof(RtMotion) * (size_t)M);
    d.o_state = (unsigned)sc.out(mn);
    d.o_cos = (unsigned)sc.out(sizeof(float) * mn);
    d.o_p3d = (unsigned)sc.out(sizeof(float) * 3 * mn);
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_init_check_rt, dim3((unsigned)((n + MT - 1) / MT), (unsigned)M), dim3(MT), 0, sc.stream(), d, sc.d<char>(0));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_init_waits.store(sc.waits, std::memory_order_relaxed);
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    const uint8_t *state = sc.r<uint8_t>(d.o_state);
    const float *cosp = sc.r<float>(d.o_cos), *p3d = sc.r<float>(d.o_p3d);
    std::vector<float> cosines;
    for (int m = 0; m < M; ++m) {
        cosines.clear();
        for (int i = 0; i < n; ++i) {                                   // in match order, as the loop of :830-894 writes
            const size_t o = (size_t)m * n + i;
            const size_t first = (size_t)m * n1 + matches[2 * i];
            if (state[o] == RT_NOT_FINITE) good[first] = 0;             // :843
            if (state[o] < RT_COUNTED) continue;
            cosines.push_back(cosp[o]);
            memcpy(P3D + 3 * first, p3d + 3 * o, sizeof(float) * 3);
            if (state[o] == RT_GOOD) good[first] = 1;
            if (counted) counted[o] = 1;
            if (cos_parallax) cos_parallax[o] = cosp[o];
        }
        ngood[m] = (int32_t)cosines.size();
        if (!cosines.empty()) {                                         // :896-902: acos(float) is acosf; float * int, then / CV_PI in double
            std::sort(cosines.begin(), cosines.end());
            const size_t idx = (size_t)std::min(50, (int)(cosines.size() - 1));
            parallax[m] = (float)((double)(acosf(cosines[idx]) * 180) / 3.1415926535897932384626433832795);
        }
    }
    return ORBX_OK;
}

int orbm_init_reconstruct_f(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n, const uint8_t *inliers,
                            const float *F21, const float *K, float sigma, float min_parallax, int min_triangulated,
                            orbm_init_reconstruction *out, float *P3D, uint8_t *triangulated)
{
    g_last_init_waits.store(0, std::memory_order_relaxed);
    if (!out || !F21 || !K || !P3D || !triangulated || (n > 0 && !inliers)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (!(sigma > 0)) ORBX_FAIL(ORBX_ERR_ARG, "sigma must be positive");
    if (const int rc = check_matches(keys1, n1, keys2, n2, matches, n)) return rc;
    memset(out, 0, sizeof(*out));
    out->best = -1;
    memset(P3D, 0, sizeof(float) * 3 * (size_t)n1);
    memset(triangulated, 0, (size_t)n1);
    int N = 0;
    for (int i = 0; i < n; ++i) N += inliers[i] != 0;
    out->N = N;
    // E21 = K.t() * F21 * K (the transposed operand materialised, float row sums)
    float Kt[9], tmp[9], E[9], w[3], u[9], vt[9];
    transpose3(K, Kt);
    orbm_svd::gemm33(Kt, F21, tmp);
    orbm_svd::gemm33(tmp, K, E);
    // DecomposeE (:909-929)
    orbm_svd::svd33(E, w, u, vt);
    float tv[3] = {u[2], u[5], u[8]}, t1[3], t2[3];
    const double nrm = sqrt((double)tv[0] * tv[0] + (double)tv[1] * tv[1] + (double)tv[2] * tv[2]);
    scale_mat(tv, 3, 1.0 / nrm, t1);
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    float Wt[9], R1[9], R2[9];
    transpose3(W, Wt);
    orbm_svd::gemm33(u, W, tmp); orbm_svd::gemm33(tmp, vt, R1);
    if (orbm_svd::det33(R1) < 0) scale_mat(R1, 9, -1.0, R1);
    orbm_svd::gemm33(u, Wt, tmp); orbm_svd::gemm33(tmp, vt, R2);
    if (orbm_svd::det33(R2) < 0) scale_mat(R2, 9, -1.0, R2);
    scale_mat(t1, 3, -1.0, t2);
    float Rs[36], ts[12];
    for (int m = 0; m < 4; ++m) {                                       // (R1, t) (R2, t) (R1, -t) (R2, -t)
        memcpy(Rs + 9 * m, (m & 1) ? R2 : R1, sizeof(R1));
        memcpy(ts + 3 * m, (m & 2) ? t2 : t1, sizeof(t1));
    }
    const float mSigma2 = sigma * sigma;
    std::vector<uint8_t> good((size_t)4 * std::max(n1, 1));
    std::vector<float> p3d((size_t)12 * std::max(n1, 1));
    const int rc = orbm_init_check_rt(keys1, n1, keys2, n2, matches, n, inliers, K, Rs, ts, 4, (float)(1.0 * mSigma2), good.data(), p3d.data(),
                                      nullptr, nullptr, out->ngood, out->parallax);
    if (rc) return rc;
    const int *g = out->ngood;
    const int maxGood = std::max(g[0], std::max(g[1], std::max(g[2], g[3])));
    const int nMinGood = std::max((int)(0.9 * N), min_triangulated);
    int nsimilar = 0;
    for (int m = 0; m < 4; ++m) nsimilar += g[m] > 0.7 * maxGood;
    out->max_good = maxGood; out->nsimilar = nsimilar;
    if (maxGood < nMinGood || nsimilar > 1) return ORBX_OK;
    int best = 0;                                                       // the == cascade: the first of equal bests, and only that one
    while (g[best] != maxGood) ++best;
    out->best = best;
    if (out->parallax[best] > min_parallax) {
        out->found = 1;
        memcpy(out->R21, Rs + 9 * best, sizeof(out->R21));
        memcpy(out->t21, ts + 3 * best, sizeof(out->t21));
        memcpy(P3D, p3d.data() + (size_t)3 * best * n1, sizeof(float) * 3 * (size_t)n1);
        memcpy(triangulated, good.data() + (size_t)best * n1, (size_t)n1);
    }
    return ORBX_OK;
}

int orbm_debug_init_svd(int shape, const float *A, float *w, float *u, float *vt)
{
    if (!A || !vt) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    switch (shape) {
    case 0: {                                                           // 16 x 9 row-major -> vt.row(8)
        float At[9][16];
        for (int r = 0; r < 16; ++r) for (int c = 0; c < 9; ++c) At[c][r] = A[9 * r + c];
        orbm_svd::svd_16x9_vt8(At, vt);
        return ORBX_OK;
    }
    case 1: {                                                           // 8 x 9 row-major -> vt.row(8)
        float At[9][9];
        for (int r = 0; r < 8; ++r) for (int c = 0; c < 9; ++c) At[r][c] = A[9 * r + c];
        for (int c = 0; c < 9; ++c) At[8][c] = 0.0f;
        orbm_svd::svd_8x9_vt8(At, vt);
        return ORBX_OK;
    }
    case 2:                                                             // 3 x 3 -> w, u, vt
        if (!w || !u) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        orbm_svd::svd33(A, w, u, vt);
        return ORBX_OK;
    case 3: {                                                           // 4 x 4 row-major -> vt.row(3)
        float At[4][4];
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) At[c][r] = A[4 * r + c];
        orbm_svd::svd_4x4_vt3(At, vt);
        return ORBX_OK;
    }
    }
    ORBX_FAIL(ORBX_ERR_ARG, "unknown shape");
}

int orbm_debug_last_init_waits(void) { return g_last_init_waits.load(std::memory_order_relaxed); }

} // extern "C"
