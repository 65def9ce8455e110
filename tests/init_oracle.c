/* CPU restatement of the monocular Initializer (src/Initializer.cc) for the tests: sequential loops, literal, one hypothesis after
 * the other (test infrastructure: never part of the product).  cv::Mat arithmetic with OpenCV 3.4's semantics as oracle/match_oracle.c
 * and tests/sim3_oracle.c have them (no OpenCV exists for this project to run: unpinned):
 *   A * B (3 x 3, 3 x 4)   gemm's small-matrix case: the float row sum left to right, then float(double(sum) * alpha + double(c) * beta);
 *                          a transposed operand is materialised first
 *   cv::invert 3 x 3       determinant and cofactors in double, one 1. / d, stored as float; all zero when d == 0
 *   cv::determinant 3 x 3  the same determinant, in double
 *   s * row - row          addWeighted with float weights: a * s + b * -1.0f
 *   v / s, -v              convertTo with a FLOAT scale: v * float(1.0 / double(s)) + 0.0f, v * -1.0f + 0.0f
 *   cv::norm, Mat::dot     double sums of double products, k ascending (three entries: below the groups of four)
 *   cv::SVDecomp           _SVDcompute + JacobiSVDImpl_<float> (modules/core/src/lapack.cpp) in its general (m, n, n1) form,
 *                          the tail with cv::RNG(0x12345678) included
 * Built with -ffp-contract=off -fno-fast-math (tests/c_oracle.py). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define IO_PI 3.1415926535897932384626433832795

/* ---------------------------------------------------------------------------------------------- cv::RNG */
static unsigned rng_next(uint64_t *state)
{
    *state = (uint64_t)(unsigned)*state * 4164903690U + (unsigned)(*state >> 32);
    return (unsigned)*state;
}

void io_rng_outputs(uint64_t seed, int count, uint32_t *out)
{
    uint64_t s = seed;
    for (int i = 0; i < count; ++i) out[i] = rng_next(&s);
}

/* ---------------------------------------------------------------------------------------------- JacobiSVDImpl_<float>
 * At: n1 rows (the first n hold the matrix, the others are zero) of astep floats, m used; Vt: n rows of vstep floats. */
static int jacobi_svd(float *At, size_t astep, float *_W, float *Vt, size_t vstep, int m, int n, int n1)
{
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    double *W = (double *)malloc(sizeof(double) * (size_t)n);
    int i, j, k, iter, max_iter = m > 30 ? m : 30, sweeps = 0;
    float c, s;
    double sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { float t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = sd;
        if (Vt) {
            for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }
    for (iter = 0; iter < max_iter; iter++) {
        int changed = 0;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                float *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt((double)a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = hypot((double)p, beta);
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    float t0 = c * Ai[k] + s * Aj[k];
                    float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = 1;
                if (Vt) {
                    float *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                    for (k = 0; k < n; k++) {
                        float t0 = c * Vi[k] + s * Vj[k];
                        float t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        sweeps++;
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { float t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double tw = W[i]; W[i] = W[j]; W[j] = tw;
            if (Vt) {
                for (k = 0; k < m; k++) { float t = At[i * astep + k]; At[i * astep + k] = At[j * astep + k]; At[j * astep + k] = t; }
                for (k = 0; k < n; k++) { float t = Vt[i * vstep + k]; Vt[i * vstep + k] = Vt[j * vstep + k]; Vt[j * vstep + k] = t; }
            }
        }
    }
    for (i = 0; i < n; i++) _W[i] = (float)W[i];
    if (!Vt) { free(W); return sweeps; }
    uint64_t rng = 0x12345678;
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            /* a zero singular value: a random vector, the earlier rows projected out, normalised */
            const float val0 = (float)(1. / m);
            for (k = 0; k < m; k++) {
                float val = (rng_next(&rng) & 256) != 0 ? val0 : -val0;
                At[i * astep + k] = val;
            }
            for (iter = 0; iter < 2; iter++) {
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    float asum = 0;
                    for (k = 0; k < m; k++) {
                        float t = (float)(At[i * astep + k] - sd * At[j * astep + k]);
                        At[i * astep + k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            }
            sd = 0;
            for (k = 0; k < m; k++) { float t = At[i * astep + k]; sd += (double)t * t; }
            sd = sqrt(sd);
        }
        s = (float)(sd > minval ? 1 / sd : 0.);
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
    free(W);
    return sweeps;
}

/* _SVDcompute: cv::SVDecomp(src, w, u, vt, flags) of a rows x cols float matrix, always with u and vt.  w [min(rows, cols)];
 * rows >= cols: u [rows][urows], vt [cols][cols]; rows < cols: u [rows][rows], vt [urows][cols]; urows = full_uv ? max : min.
 * Returns the number of sweeps. */
int io_svdecomp(const float *src, int rows, int cols, int full_uv, float *w, float *u, float *vt)
{
    int m = rows, n = cols, at = 0;
    if (m < n) { int t = m; m = n; n = t; at = 1; }
    const int urows = full_uv ? m : n;
    float *temp_u = (float *)calloc((size_t)urows * m, sizeof(float));     /* temp_a = its first n rows */
    float *temp_v = (float *)calloc((size_t)n * n, sizeof(float));
    if (!at) { for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) temp_u[c * m + r] = src[r * cols + c]; }
    else memcpy(temp_u, src, sizeof(float) * (size_t)rows * cols);
    const int sweeps = jacobi_svd(temp_u, (size_t)m, w, temp_v, (size_t)n, m, n, urows);
    if (!at) {
        for (int r = 0; r < urows; r++) for (int c = 0; c < m; c++) u[c * urows + r] = temp_u[r * m + c];
        memcpy(vt, temp_v, sizeof(float) * (size_t)n * n);
    } else {
        for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) u[c * n + r] = temp_v[r * n + c];
        memcpy(vt, temp_u, sizeof(float) * (size_t)urows * m);
    }
    free(temp_u); free(temp_v);
    return sweeps;
}

/* ---------------------------------------------------------------------------------------------- cv::Mat pieces, 3 x 3 */
static void gemm33(const float *A, const float *B, float *D)
{
    float out[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            float t = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
            out[3 * r + c] = (float)((double)t * 1.0 + (double)0.0f * 0.0);
        }
    memcpy(D, out, sizeof(out));
}

static void transpose33(const float *A, float *At)
{
    float out[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out[3 * r + c] = A[3 * c + r];
    memcpy(At, out, sizeof(out));
}

static double det33(const float *m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

void io_invert33(const float *S, float *Dst)
{
    double d = det33(S);
    float out[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
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
    }
    memcpy(Dst, out, sizeof(out));
}

static void scale_vec(const float *v, int n, double s, float *out)
{
    const float a = (float)s, b = (float)0.0;
    for (int i = 0; i < n; i++) out[i] = v[i] * a + b;
}

/* ---------------------------------------------------------------------------------------------- Normalize :749-795 */
void io_normalize(const float *keys, int N, float *pn, float *T)
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; i++) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) {
        pn[2 * i] = keys[2 * i] - meanX; pn[2 * i + 1] = keys[2 * i + 1] - meanY;
        meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
    }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    float sX = (float)(1.0 / meanDevX), sY = (float)(1.0 / meanDevY);
    for (int i = 0; i < N; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    for (int k = 0; k < 9; k++) T[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    T[0] = sX; T[4] = sY; T[2] = -meanX * sX; T[5] = -meanY * sY;
}

/* ---------------------------------------------------------------------------------------------- ComputeH21 :226-266, ComputeF21 :268-303
 * p1, p2: [8][2] */
void io_compute_h21(const float *p1, const float *p2, float *H)
{
    float A[16 * 9], w[9], u[16 * 16], vt[9 * 9];
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        float *r0 = A + 9 * (2 * i), *r1 = A + 9 * (2 * i + 1);
        r0[0] = 0.0; r0[1] = 0.0; r0[2] = 0.0; r0[3] = -u1; r0[4] = -v1; r0[5] = -1; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
        r1[0] = u1; r1[1] = v1; r1[2] = 1; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0; r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
    }
    io_svdecomp(A, 16, 9, 1, w, u, vt);
    memcpy(H, vt + 9 * 8, sizeof(float) * 9);
}

void io_compute_f21(const float *p1, const float *p2, float *F)
{
    float A[8 * 9], w[8], u[8 * 8], vt[9 * 9], Fpre[9], w3[3], u3[9], vt3[9], tmp[9];
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        float *r = A + 9 * i;
        r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
    }
    io_svdecomp(A, 8, 9, 1, w, u, vt);
    memcpy(Fpre, vt + 9 * 8, sizeof(Fpre));
    io_svdecomp(Fpre, 3, 3, 1, w3, u3, vt3);
    w3[2] = 0;
    const float dg[9] = {w3[0], 0, 0, 0, w3[1], 0, 0, 0, w3[2]};
    gemm33(u3, dg, tmp);
    gemm33(tmp, vt3, F);
}

/* ---------------------------------------------------------------------------------------------- CheckHomography :305-388
 * chi [n][2]: the chiSquare1 / chiSquare2 compared */
float io_check_homography(const float *H21, const float *H12, const float *keys1, const float *keys2, const int32_t *matches, int N,
                          float sigma, uint8_t *inliers, float *chi)
{
    const float h11 = H21[0], h12 = H21[1], h13 = H21[2], h21 = H21[3], h22 = H21[4], h23 = H21[5], h31 = H21[6], h32 = H21[7], h33 = H21[8];
    const float h11inv = H12[0], h12inv = H12[1], h13inv = H12[2], h21inv = H12[3], h22inv = H12[4], h23inv = H12[5], h31inv = H12[6],
                h32inv = H12[7], h33inv = H12[8];
    float score = 0;
    const float th = 5.991;
    const float invSigmaSquare = 1.0 / (sigma * sigma);
    for (int i = 0; i < N; i++) {
        int bIn = 1;
        const float u1 = keys1[2 * matches[2 * i]], v1 = keys1[2 * matches[2 * i] + 1];
        const float u2 = keys2[2 * matches[2 * i + 1]], v2 = keys2[2 * matches[2 * i + 1] + 1];
        const float w2in1inv = 1.0 / (h31inv * u2 + h32inv * v2 + h33inv);
        const float u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv;
        const float v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv;
        const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = 0; else score += th - chiSquare1;
        const float w1in2inv = 1.0 / (h31 * u1 + h32 * v1 + h33);
        const float u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv;
        const float v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv;
        const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = 0; else score += th - chiSquare2;
        inliers[i] = bIn ? 1 : 0;
        if (chi) { chi[2 * i] = chiSquare1; chi[2 * i + 1] = chiSquare2; }
    }
    return score;
}

/* CheckFundamental :390-468 */
float io_check_fundamental(const float *F21, const float *keys1, const float *keys2, const int32_t *matches, int N, float sigma,
                           uint8_t *inliers, float *chi)
{
    const float f11 = F21[0], f12 = F21[1], f13 = F21[2], f21 = F21[3], f22 = F21[4], f23 = F21[5], f31 = F21[6], f32 = F21[7], f33 = F21[8];
    float score = 0;
    const float th = 3.841;
    const float thScore = 5.991;
    const float invSigmaSquare = 1.0 / (sigma * sigma);
    for (int i = 0; i < N; i++) {
        int bIn = 1;
        const float u1 = keys1[2 * matches[2 * i]], v1 = keys1[2 * matches[2 * i] + 1];
        const float u2 = keys2[2 * matches[2 * i + 1]], v2 = keys2[2 * matches[2 * i + 1] + 1];
        const float a2 = f11 * u1 + f12 * v1 + f13;
        const float b2 = f21 * u1 + f22 * v1 + f23;
        const float c2 = f31 * u1 + f32 * v1 + f33;
        const float num2 = a2 * u2 + b2 * v2 + c2;
        const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = 0; else score += thScore - chiSquare1;
        const float a1 = f11 * u2 + f21 * v2 + f31;
        const float b1 = f12 * u2 + f22 * v2 + f32;
        const float c1 = f13 * u2 + f23 * v2 + f33;
        const float num1 = a1 * u1 + b1 * v1 + c1;
        const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = 0; else score += thScore - chiSquare2;
        inliers[i] = bIn ? 1 : 0;
        if (chi) { chi[2 * i] = chiSquare1; chi[2 * i + 1] = chiSquare2; }
    }
    return score;
}

/* ---------------------------------------------------------------------------------------------- FindHomography :124-172 (model 0),
 * FindFundamental :175-223 (model 1).  hyp_* (each may be NULL): per iteration the matrix [H][9], the score [H], the flags [H][n]
 * and the compared chiSquares [H][n][2].  best_*: what the function returns; best_it = the winning iteration, -1 = none (the
 * flags are then n falses for H; the reference leaves F's vector EMPTY, reported here as zeros and best_it = -1). */
void io_find_model(int model, const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n, const int32_t *sets,
                   int H, float sigma, float *hyp_mat, float *hyp_score, uint8_t *hyp_flags, float *hyp_chi, float *best_mat,
                   float *best_score, uint8_t *best_flags, int32_t *best_it)
{
    float *vPn1 = (float *)malloc(sizeof(float) * 2 * (size_t)(n1 > 0 ? n1 : 1)), *vPn2 = (float *)malloc(sizeof(float) * 2 * (size_t)(n2 > 0 ? n2 : 1));
    float T1[9], T2[9], T2inv[9], T2t[9];
    io_normalize(keys1, n1, vPn1, T1);
    io_normalize(keys2, n2, vPn2, T2);
    io_invert33(T2, T2inv);
    transpose33(T2, T2t);
    float score = 0.0;
    uint8_t *cur = (uint8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
    float *chi = (float *)calloc((size_t)(n > 0 ? n : 1) * 2, sizeof(float));
    memset(best_flags, 0, (size_t)n);
    memset(best_mat, 0, sizeof(float) * 9);
    *best_it = -1;
    for (int it = 0; it < H; it++) {
        float p1[16], p2[16], Mn[9], Mi[9], Minv[9], tmp[9];
        for (int j = 0; j < 8; j++) {
            const int idx = sets[8 * it + j];
            p1[2 * j] = vPn1[2 * matches[2 * idx]]; p1[2 * j + 1] = vPn1[2 * matches[2 * idx] + 1];
            p2[2 * j] = vPn2[2 * matches[2 * idx + 1]]; p2[2 * j + 1] = vPn2[2 * matches[2 * idx + 1] + 1];
        }
        float currentScore;
        if (model == 0) {
            io_compute_h21(p1, p2, Mn);
            gemm33(T2inv, Mn, tmp); gemm33(tmp, T1, Mi);
            io_invert33(Mi, Minv);
            currentScore = io_check_homography(Mi, Minv, keys1, keys2, matches, n, sigma, cur, chi);
        } else {
            io_compute_f21(p1, p2, Mn);
            gemm33(T2t, Mn, tmp); gemm33(tmp, T1, Mi);
            currentScore = io_check_fundamental(Mi, keys1, keys2, matches, n, sigma, cur, chi);
        }
        if (hyp_mat) memcpy(hyp_mat + 9 * (size_t)it, Mi, sizeof(Mi));
        if (hyp_score) hyp_score[it] = currentScore;
        if (hyp_flags) memcpy(hyp_flags + (size_t)it * n, cur, (size_t)n);
        if (hyp_chi) memcpy(hyp_chi + (size_t)it * n * 2, chi, sizeof(float) * 2 * (size_t)n);
        if (currentScore > score) {
            memcpy(best_mat, Mi, sizeof(Mi));
            memcpy(best_flags, cur, (size_t)n);
            score = currentScore;
            *best_it = it;
        }
    }
    *best_score = score;
    free(vPn1); free(vPn2); free(cur); free(chi);
}

/* ---------------------------------------------------------------------------------------------- Triangulate :734-747 */
static void triangulate(float x1, float y1, float x2, float y2, const float *P1, const float *P2, float *x3D)
{
    float A[16], w[4], u[16], vt[16];
    for (int c = 0; c < 4; c++) {
        A[c] = x1 * P1[8 + c] + P1[c] * -1.0f;
        A[4 + c] = y1 * P1[8 + c] + P1[4 + c] * -1.0f;
        A[8 + c] = x2 * P2[8 + c] + P2[c] * -1.0f;
        A[12 + c] = y2 * P2[8 + c] + P2[4 + c] * -1.0f;
    }
    io_svdecomp(A, 4, 4, 1, w, u, vt);
    const float inv = (float)(1.0 / (double)vt[15]);
    x3D[0] = vt[12] * inv; x3D[1] = vt[13] * inv; x3D[2] = vt[14] * inv;
}

/* vt.row(3) of a 4 x 4 float matrix (the instantiation Triangulate uses) */
int io_svd_vt3(const float *A, float *v)
{
    float w[4], u[16], vt[16];
    const int sweeps = io_svdecomp(A, 4, 4, 1, w, u, vt);
    memcpy(v, vt + 12, sizeof(float) * 4);
    return sweeps;
}

/* ---------------------------------------------------------------------------------------------- CheckRT :798-907
 * good [n1], P3D [n1][3] (zeroed here: what the reference never writes stays 0); per match counted [n], cosp [n] and err [n][2] =
 * squareError1 / squareError2 where the loop got as far as computing them (else -1). */
int io_check_rt(const float *R, const float *t, const float *keys1, int n1, const float *keys2, const int32_t *matches, int n,
                const uint8_t *inliers, const float *K, float *P3D, float th2, uint8_t *good, float *parallax, uint8_t *counted, float *cosp,
                float *err)
{
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    memset(good, 0, (size_t)n1);
    memset(P3D, 0, sizeof(float) * 3 * (size_t)n1);
    float *vCos = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    int ncos = 0;
    float P1[12], P2[12], O2[3], Rt[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) P1[4 * r + c] = c < 3 ? K[3 * r + c] : 0.0f;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            const float s = K[3 * r] * b0 + K[3 * r + 1] * b1 + K[3 * r + 2] * b2;
            P2[4 * r + c] = (float)((double)s * 1.0 + (double)0.0f * 0.0);
        }
    transpose33(R, Rt);
    for (int k = 0; k < 3; k++) {                                       /* O2 = -R.t() * t: one gemm with alpha = -1 */
        const float s = Rt[3 * k] * t[0] + Rt[3 * k + 1] * t[1] + Rt[3 * k + 2] * t[2];
        O2[k] = (float)((double)s * -1.0 + (double)0.0f * 0.0);
    }
    int nGood = 0;
    for (int i = 0; i < n; i++) {
        if (counted) counted[i] = 0;
        if (cosp) cosp[i] = 0;
        if (err) { err[2 * i] = -1; err[2 * i + 1] = -1; }
        if (!inliers[i]) continue;
        const int first = matches[2 * i];
        const float x1 = keys1[2 * first], y1 = keys1[2 * first + 1], x2 = keys2[2 * matches[2 * i + 1]], y2 = keys2[2 * matches[2 * i + 1] + 1];
        float p[3];
        triangulate(x1, y1, x2, y2, P1, P2, p);
        if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) { good[first] = 0; continue; }
        float normal1[3], normal2[3];
        for (int k = 0; k < 3; k++) { normal1[k] = p[k] - 0.0f; normal2[k] = p[k] - O2[k]; }
        double s1 = 0, s2 = 0, dt = 0;
        for (int k = 0; k < 3; k++) { s1 += (double)normal1[k] * normal1[k]; s2 += (double)normal2[k] * normal2[k]; dt += (double)normal1[k] * normal2[k]; }
        float dist1 = sqrt(s1), dist2 = sqrt(s2);
        float cosParallax = dt / (dist1 * dist2);
        if (p[2] <= 0 && cosParallax < 0.9998) continue;
        float p2[3];
        for (int r = 0; r < 3; r++)
            p2[r] = (float)((double)(R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) * 1.0 + (double)t[r] * 1.0);
        if (p2[2] <= 0 && cosParallax < 0.9998) continue;
        float invZ1 = 1.0 / p[2];
        float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
        float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
        if (err) err[2 * i] = squareError1;
        if (squareError1 > th2) continue;
        float invZ2 = 1.0 / p2[2];
        float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
        float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
        if (err) err[2 * i + 1] = squareError2;
        if (squareError2 > th2) continue;
        vCos[ncos++] = cosParallax;
        P3D[3 * first] = p[0]; P3D[3 * first + 1] = p[1]; P3D[3 * first + 2] = p[2];
        nGood++;
        if (counted) counted[i] = 1;
        if (cosp) cosp[i] = cosParallax;
        if (cosParallax < 0.9998) good[first] = 1;
    }
    if (nGood > 0) {
        for (int a = 1; a < ncos; a++) {                                /* sort ascending */
            float v = vCos[a]; int b = a - 1;
            while (b >= 0 && vCos[b] > v) { vCos[b + 1] = vCos[b]; b--; }
            vCos[b + 1] = v;
        }
        int idx = 50 < ncos - 1 ? 50 : ncos - 1;
        *parallax = (float)((double)(acosf(vCos[idx]) * 180) / IO_PI);   /* acos(float) * int, then / CV_PI in double */
    } else
        *parallax = 0;
    free(vCos);
    return nGood;
}

/* ---------------------------------------------------------------------------------------------- DecomposeE :909-929 */
void io_decompose_e(const float *E, float *R1, float *R2, float *t)
{
    float w[3], u[9], vt[9], tmp[9];
    io_svdecomp(E, 3, 3, 0, w, u, vt);
    float tv[3] = {u[2], u[5], u[8]};
    const double nrm = sqrt((double)tv[0] * tv[0] + (double)tv[1] * tv[1] + (double)tv[2] * tv[2]);
    scale_vec(tv, 3, 1.0 / nrm, t);
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    float Wt[9];
    transpose33(W, Wt);
    gemm33(u, W, tmp); gemm33(tmp, vt, R1);
    if (det33(R1) < 0) scale_vec(R1, 9, -1.0, R1);
    gemm33(u, Wt, tmp); gemm33(tmp, vt, R2);
    if (det33(R2) < 0) scale_vec(R2, 9, -1.0, R2);
}

/* ---------------------------------------------------------------------------------------------- ReconstructF :470-570
 * Returns found; ngood [4], parallax [4]; best = the motion the == cascade looked at (-1: rejected before). */
int io_reconstruct_f(const uint8_t *inliers, const float *F21, const float *K, const float *keys1, int n1, const float *keys2,
                     const int32_t *matches, int n, float sigma, float minParallax, int minTriangulated, float *R21, float *t21, float *P3D,
                     uint8_t *triangulated, int32_t *ngood, float *parallax, int32_t *best)
{
    int N = 0;
    for (int i = 0; i < n; i++) if (inliers[i]) N++;
    float Kt[9], tmp[9], E21[9], R1[9], R2[9], t1[3], t2[3];
    transpose33(K, Kt);
    gemm33(Kt, F21, tmp); gemm33(tmp, K, E21);
    io_decompose_e(E21, R1, R2, t1);
    scale_vec(t1, 3, -1.0, t2);
    const float mSigma2 = sigma * sigma;
    const size_t m1 = (size_t)(n1 > 0 ? n1 : 1);
    float *p3 = (float *)calloc(4 * 3 * m1, sizeof(float));
    uint8_t *gd = (uint8_t *)calloc(4 * m1, 1);
    const float *Rs[4] = {R1, R2, R1, R2}, *ts[4] = {t1, t1, t2, t2};
    for (int m = 0; m < 4; m++)
        ngood[m] = io_check_rt(Rs[m], ts[m], keys1, n1, keys2, matches, n, inliers, K, p3 + 3 * m1 * m, 1.0 * mSigma2, gd + m1 * m, parallax + m, NULL,
                               NULL, NULL);
    int maxGood = ngood[0];
    for (int m = 1; m < 4; m++) if (ngood[m] > maxGood) maxGood = ngood[m];
    memset(R21, 0, sizeof(float) * 9); memset(t21, 0, sizeof(float) * 3);
    memset(P3D, 0, sizeof(float) * 3 * (size_t)n1); memset(triangulated, 0, (size_t)n1);
    *best = -1;
    int nMinGood = (int)(0.9 * N) > minTriangulated ? (int)(0.9 * N) : minTriangulated;
    int nsimilar = 0;
    for (int m = 0; m < 4; m++) if (ngood[m] > 0.7 * maxGood) nsimilar++;
    int found = 0;
    if (!(maxGood < nMinGood || nsimilar > 1)) {
        int b = 0;
        while (ngood[b] != maxGood) b++;
        *best = b;
        if (parallax[b] > minParallax) {
            memcpy(P3D, p3 + 3 * m1 * b, sizeof(float) * 3 * (size_t)n1);
            memcpy(triangulated, gd + m1 * b, (size_t)n1);
            memcpy(R21, Rs[b], sizeof(float) * 9); memcpy(t21, ts[b], sizeof(float) * 3);
            found = 1;
        }
    }
    free(p3); free(gd);
    return found;
}

/* ---------------------------------------------------------------------------------------------- Initialize :44-121
 * vMatches12 [n1]; sets [H][8] pre-drawn.  Status: 0 not initialised, 1 initialised, 2 RH > 0.99 (the reference goes on to
 * ReconstructH, which is not restated), 3 no fundamental matrix (the reference would throw in ReconstructF).  matches_out [n1][2]
 * (the first *n_out rows). */
int io_initialize(const float *keys1, int n1, const float *keys2, int n2, const int32_t *vMatches12, const int32_t *sets, int H, float sigma,
                  const float *K, int32_t *matches_out, int32_t *n_out, float *RH_out, float *R21, float *t21, float *P3D, uint8_t *triangulated)
{
    int n = 0;
    for (int i = 0; i < n1; i++)
        if (vMatches12[i] >= 0) { matches_out[2 * n] = i; matches_out[2 * n + 1] = vMatches12[i]; n++; }
    *n_out = n;
    const size_t m = (size_t)(n > 0 ? n : 1);
    uint8_t *inH = (uint8_t *)calloc(m, 1), *inF = (uint8_t *)calloc(m, 1);
    float Hm[9], Fm[9], SH, SF;
    int32_t itH, itF;
    io_find_model(0, keys1, n1, keys2, n2, matches_out, n, sets, H, sigma, NULL, NULL, NULL, NULL, Hm, &SH, inH, &itH);
    io_find_model(1, keys1, n1, keys2, n2, matches_out, n, sets, H, sigma, NULL, NULL, NULL, NULL, Fm, &SF, inF, &itF);
    float RH = SH / (SH + SF);
    *RH_out = RH;
    int status;
    memset(R21, 0, sizeof(float) * 9); memset(t21, 0, sizeof(float) * 3);
    memset(P3D, 0, sizeof(float) * 3 * (size_t)n1); memset(triangulated, 0, (size_t)n1);
    if (RH > 0.99) status = 2;
    else if (itF < 0) status = 3;
    else {
        int32_t ngood[4], best;
        float parallax[4];
        status = io_reconstruct_f(inF, Fm, K, keys1, n1, keys2, matches_out, n, sigma, 0.95, 60, R21, t21, P3D, triangulated, ngood, parallax, &best);
    }
    free(inH); free(inF);
    return status;
}
