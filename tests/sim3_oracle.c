/* sim3_oracle.c -- CPU restatement of Sim3Solver (src/Sim3Solver.cc) over flat arrays.  Test infrastructure: never part of the
 * product.  tests/sim3_oracle.py is its ctypes wrapper.
 *
 * Restated, with the reference's float / double order op by op:
 *   s3o_prepare          the constructor's data preparation (:54-109): X3Dc = Rcw * Xw + tcw, FromCameraToImage (:405-423), and the
 *                        integer thresholds mvnMaxError1/2 (:87-88)
 *   s3o_compute_sim3     ComputeCentroid (:215-224) and ComputeSim3 (:226-337)
 *   s3o_hypotheses       per drawn triple: ComputeSim3, Project (:382-403), CheckInliers (:340-364)
 *   s3o_ransac_max_its   SetRansacParameters (:114-138)
 *   s3o_iterate          the fold of iterate (:140-207) over per-hypothesis inlier counts
 *
 * cv::Mat arithmetic (OpenCV 3.4, CV_32F; OpenCV is not available to this project, so parity with it is unpinned, like the other
 * OpenCV primitives of DESIGN section 5), with the semantics of oracle/match_oracle.c:
 *   A * b (+ c)            gemm's 3 x 3 case: t = a0 b0 + a1 b1 + a2 b2 in float, left to right, d = float(double(t) * alpha +
 *                          double(c) * beta); A * B.t(): the transposed matrix materialised, then the same row sums;
 *                          O1 - s * R * O2 is ONE gemm with alpha = -double(s), c = O1, beta = 1 (MatOp_GEMM::subtract)
 *   Mat / int, double*Mat  convertTo with a FLOAT scale: a * float(alpha) + 0.0f; 2*ang*vec/norm(vec) is one scale with
 *                          alpha = (2 * ang) * (1.0 / norm) in double
 *   cv::reduce(SUM, dim 1) of a row of three floats (ReduceC_Invoker): (p0 + p2) + p1 in float
 *   A - B, cv::pow(A, 2)   float subtraction, float a * a
 *   cv::norm               sqrt of the double sum of double squares, left to right
 *   Mat::dot               dotProd_: double products, summed in groups of four ((p0 + p1) + p2) + p3, each group added to the
 *                          running sum, the remainder one by one (nine entries: two groups and one; two or three entries: one by one)
 *   cv::eigen              on a 4 x 4 symmetric float matrix: JacobiImpl_<float> (modules/core/src/lapack.cpp): the largest
 *                          off-diagonal element of the upper triangle as pivot, tracked through indR / indC exactly as the
 *                          original does (stale entries included), its own float hypot, stop at |p| <= FLT_EPSILON or after
 *                          n * n * 30 = 480 rotations, then eigenvalues sorted descending with their rows
 *   cv::Rodrigues          vector -> matrix (cvRodrigues2): in double, theta = sqrt(x x + y y + z z); theta < DBL_EPSILON gives
 *                          the identity; else R = c I + (1 - c) r r^T + s [r]x per element as (c * I + c1 * rrt) + s * rx, then
 *                          rounded to float
 * The identity rotation: the leading eigenvector is (+-1, 0, 0, 0), norm(vec) = 0, alpha = (2 * ang) * (1.0 / 0.0) is NaN (ang = 0)
 * or inf (ang = pi), 0.0f * float(alpha) is NaN either way, so Rodrigues is handed (NaN, NaN, NaN): theta is NaN, `theta <
 * DBL_EPSILON` is false, and R, s, t, T12 are all NaN.  Every comparison in CheckInliers is then false: 0 inliers.  The restated
 * Rodrigues does exactly that (s3o_rodrigues of a NaN vector = a NaN matrix).
 *
 * Every flag of CheckInliers also records its GAP: the smaller of |err - max| / max(|err|, max) over the two comparisons (1 where
 * an error is not finite: such a flag is robustly "out").
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -std=c99 -shared -fPIC. */
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------------ cv::Mat pieces */
static float row3(const float *R, int r, float b0, float b1, float b2) { return R[3 * r] * b0 + R[3 * r + 1] * b1 + R[3 * r + 2] * b2; }
static float gemm_out(float t, double alpha, float c, double beta) { return (float)((double)t * alpha + (double)c * beta); }

/* cv::hypot of lapack.cpp (a template in float, not the C library's) */
static float cv_hypotf(float a, float b)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}

/* cv::eigen(N, eval, evec) of a 4 x 4 symmetric CV_32F matrix: eval descending, evec rows.  Returns the number of rotations. */
int s3o_eigen4(const float *N16, float *W, float *V)
{
    enum { n = 4 };
    const float eps = FLT_EPSILON;
    float A[16], mv;
    int indR[n], indC[n], i, j, k, m, iters;
    const int maxIters = n * n * 30;
    memcpy(A, N16, sizeof(A));
    for (i = 0; i < n; i++) { for (j = 0; j < n; j++) V[n * i + j] = 0; V[n * i + i] = 1; }
    for (k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = fabsf(A[n * k + m]), i = k + 2; i < n; i++) { const float val = fabsf(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = fabsf(A[k]), i = 1; i < k; i++) { const float val = fabsf(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
            indC[k] = m;
        }
    }
    for (iters = 0; iters < maxIters; iters++) {
        int l;
        float p, y, t, s, c, a0, b0;
        for (k = 0, mv = fabsf(A[indR[0]]), i = 1; i < n - 1; i++) { const float val = fabsf(A[n * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
        l = indR[k];
        for (i = 1; i < n; i++) { const float val = fabsf(A[n * indC[i] + i]); if (mv < val) { mv = val; k = indC[i]; l = i; } }
        p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        y = (float)((W[l] - W[k]) * 0.5);
        t = fabsf(y) + cv_hypotf(p, y);
        s = cv_hypotf(p, t);
        c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        A[n * k + l] = 0;
        W[k] -= t;
        W[l] += t;
#define ROTATE(v0, v1) (a0 = (v0), b0 = (v1), (v0) = a0 * c - b0 * s, (v1) = a0 * s + b0 * c)
        for (i = 0; i < k; i++) ROTATE(A[n * i + k], A[n * i + l]);
        for (i = k + 1; i < l; i++) ROTATE(A[n * k + i], A[n * i + l]);
        for (i = l + 1; i < n; i++) ROTATE(A[n * k + i], A[n * l + i]);
        for (i = 0; i < n; i++) ROTATE(V[n * k + i], V[n * l + i]);
#undef ROTATE
        for (j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = fabsf(A[n * idx + m]), i = idx + 2; i < n; i++) { const float val = fabsf(A[n * idx + i]); if (mv < val) { mv = val; m = i; } }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = fabsf(A[idx]), i = 1; i < idx; i++) { const float val = fabsf(A[n * i + idx]); if (mv < val) { mv = val; m = i; } }
                indC[idx] = m;
            }
        }
    }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            const float w = W[m]; W[m] = W[k]; W[k] = w;
            for (i = 0; i < n; i++) { const float v = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = v; }
        }
    }
    return iters;
}

/* cv::Rodrigues(vec, R): 1 x 3 CV_32F -> 3 x 3 CV_32F */
void s3o_rodrigues(const float *v, float *R)
{
    double rx = v[0], ry = v[1], rz = v[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    int i;
    if (theta < DBL_EPSILON) {
        for (i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    {
        const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
        rx *= itheta; ry *= itheta; rz *= itheta;
        {
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
            for (i = 0; i < 9; i++) R[i] = (float)((c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * r_x[i]);
        }
    }
}

/* ------------------------------------------------------------------------------------------------ the constructor (:54-109) */
uint64_t s3o_max_error(float sigma2) { return (uint64_t)(9.210 * sigma2); }            /* :87: a double truncated into a size_t */
int s3o_is_inlier(float err1, float err2, uint64_t max1, uint64_t max2) { return err1 < (float)max1 && err2 < (float)max2; }   /* :356 */

static void to_image(const float *Xc, const float *cam, float *uv)                       /* FromCameraToImage :405-423 */
{
    const float invz = 1 / Xc[2];
    const float x = Xc[0] * invz, y = Xc[1] * invz;
    uv[0] = cam[0] * x + cam[2]; uv[1] = cam[1] * y + cam[3];
}

/* cam = fx, fy, cx, cy */
void s3o_prepare(const float *X1w, const float *X2w, const int32_t *oct1, const int32_t *oct2, const float *Tcw1, const float *Tcw2,
                 const float *cam1, const float *cam2, const float *sigma2, int n, float *X3Dc1, float *X3Dc2, float *P1im1,
                 float *P2im2, uint64_t *max1, uint64_t *max2)
{
    float R1[9], t1[3], R2[9], t2[3];
    int i, r, c;
    for (r = 0; r < 3; r++) {
        for (c = 0; c < 3; c++) { R1[3 * r + c] = Tcw1[4 * r + c]; R2[3 * r + c] = Tcw2[4 * r + c]; }
        t1[r] = Tcw1[4 * r + 3]; t2[r] = Tcw2[4 * r + 3];
    }
    for (i = 0; i < n; i++) {
        const float *a = X1w + 3 * i, *b = X2w + 3 * i;
        max1[i] = s3o_max_error(sigma2[oct1[i]]); max2[i] = s3o_max_error(sigma2[oct2[i]]);
        for (r = 0; r < 3; r++) {
            X3Dc1[3 * i + r] = gemm_out(row3(R1, r, a[0], a[1], a[2]), 1.0, t1[r], 1.0);     /* :95 */
            X3Dc2[3 * i + r] = gemm_out(row3(R2, r, b[0], b[1], b[2]), 1.0, t2[r], 1.0);     /* :98 */
        }
        to_image(X3Dc1 + 3 * i, cam1, P1im1 + 2 * i);
        to_image(X3Dc2 + 3 * i, cam2, P2im2 + 2 * i);
    }
}

/* ------------------------------------------------------------------------------------------------ ComputeSim3 (:226-337) */
/* P (3 x 3, column i = point i, as P3Dc1i): here p[i][3] = point i.  Pr[r][i], C[r] */
static void centroid(const float p[3][3], float Pr[3][3], float *C)                       /* :215-224 */
{
    const float third = (float)(1.0 / 3);
    int r, i;
    for (r = 0; r < 3; r++) {
        const float sum = (p[0][r] + p[2][r]) + p[1][r];                                  /* cv::reduce: a0 = p0, a1 = p1; a0 += p2; a0 += a1 */
        C[r] = sum * third + 0.0f;
        for (i = 0; i < 3; i++) Pr[r][i] = p[i][r] - C[r];
    }
}

/* p1, p2: the three points of each set, [3][3].  Out: T12[16], R12[9], t12[3], s12, T21[16]; Nout (optional): the matrix N */
void s3o_compute_sim3(const float *p1, const float *p2, int fix_scale, float *T12, float *R12, float *t12, float *s12, float *T21, float *Nout)
{
    float P1[3][3], P2[3][3], Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3], N[16], W[4], V[16], vec[3], R[9], P3[3][3], s, sR[9], sRinv[9];
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44, nrm, ang, alpha;
    int r, c, k;
    memcpy(P1, p1, sizeof(P1)); memcpy(P2, p2, sizeof(P2));
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    for (r = 0; r < 3; r++)                                                              /* M = Pr2 * Pr1.t() :243 */
        for (c = 0; c < 3; c++) M[r][c] = gemm_out(Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1] + Pr2[r][2] * Pr1[c][2], 1.0, 0.0f, 0.0);
    N11 = M[0][0] + M[1][1] + M[2][2];                                                   /* float sums, widened on assignment :251-260 */
    N12 = M[1][2] - M[2][1];
    N13 = M[2][0] - M[0][2];
    N14 = M[0][1] - M[1][0];
    N22 = M[0][0] - M[1][1] - M[2][2];
    N23 = M[0][1] + M[1][0];
    N24 = M[2][0] + M[0][2];
    N33 = -M[0][0] + M[1][1] - M[2][2];
    N34 = M[1][2] + M[2][1];
    N44 = -M[0][0] - M[1][1] + M[2][2];
    {
        const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
        for (k = 0; k < 16; k++) N[k] = (float)Nd[k];
    }
    if (Nout) memcpy(Nout, N, sizeof(N));
    s3o_eigen4(N, W, V);
    vec[0] = V[1]; vec[1] = V[2]; vec[2] = V[3];                                         /* :275 */
    nrm = sqrt((double)vec[0] * vec[0] + (double)vec[1] * vec[1] + (double)vec[2] * vec[2]);
    ang = atan2(nrm, (double)V[0]);                                                      /* :278 */
    alpha = (2 * ang) * (1. / nrm);                                                      /* :280 */
    for (k = 0; k < 3; k++) vec[k] = vec[k] * (float)alpha + 0.0f;
    s3o_rodrigues(vec, R);                                                               /* :284 */
    for (r = 0; r < 3; r++)                                                              /* P3 = R * Pr2 :288 */
        for (c = 0; c < 3; c++) P3[r][c] = gemm_out(R[3 * r] * Pr2[0][c] + R[3 * r + 1] * Pr2[1][c] + R[3 * r + 2] * Pr2[2][c], 1.0, 0.0f, 0.0);
    if (!fix_scale) {
        const float *a = &Pr1[0][0], *b = &P3[0][0];
        double nom = 0, den = 0;
        for (k = 0; k < 8; k += 4)
            nom += (double)a[k] * b[k] + (double)a[k + 1] * b[k + 1] + (double)a[k + 2] * b[k + 2] + (double)a[k + 3] * b[k + 3];
        nom += (double)a[8] * b[8];                                                      /* :294 */
        for (r = 0; r < 3; r++)
            for (c = 0; c < 3; c++) { const float sq = P3[r][c] * P3[r][c]; den += sq; } /* :297-306 */
        s = (float)(nom / den);                                                          /* :308 */
    } else
        s = 1.0f;
    for (r = 0; r < 3; r++)                                                              /* t12 = O1 - s * R * O2 :316 */
        t12[r] = gemm_out(row3(R, r, O2[0], O2[1], O2[2]), -(double)s, O1[r], 1.0);
    for (k = 0; k < 9; k++) sR[k] = R[k] * (float)(double)s + 0.0f;                      /* :323 */
    memset(T12, 0, sizeof(float) * 16); T12[15] = 1;
    for (r = 0; r < 3; r++) { for (c = 0; c < 3; c++) T12[4 * r + c] = sR[3 * r + c]; T12[4 * r + 3] = t12[r]; }
    {
        const float inv = (float)(1.0 / s);                                              /* :332 */
        for (r = 0; r < 3; r++) for (c = 0; c < 3; c++) sRinv[3 * r + c] = R[3 * c + r] * inv + 0.0f;
    }
    memset(T21, 0, sizeof(float) * 16); T21[15] = 1;
    for (r = 0; r < 3; r++) {
        for (c = 0; c < 3; c++) T21[4 * r + c] = sRinv[3 * r + c];
        T21[4 * r + 3] = gemm_out(row3(sRinv, r, t12[0], t12[1], t12[2]), -1.0, 0.0f, 0.0);   /* tinv = -sRinv * t12 :335 */
    }
    memcpy(R12, R, sizeof(R)); *s12 = s;
}

/* Project (:382-403) of one camera-frame point through T (4 x 4) and cam; no depth test */
static void project(const float *T, const float *X, const float *cam, float *uv)
{
    float P[3];
    int r;
    for (r = 0; r < 3; r++) P[r] = gemm_out(T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2], 1.0, T[4 * r + 3], 1.0);
    to_image(P, cam, uv);
}

static void gap_cmp(double *gap, double lhs, double rhs)
{
    const double m = fmax(fabs(lhs), fabs(rhs));
    const double g = m > 0 ? fabs(lhs - rhs) / m : 0.0;
    if (g < *gap) *gap = g;
}

/* H hypotheses over prepared data.  Out per hypothesis h: T12[h][16], R12[h][9], t12[h][3], s12[h], nin[h]; flags[h][n] (0 / 1),
 * gap[h][n] (optional), err[h][n][2] (optional: err1, err2) */
void s3o_hypotheses(const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2, const uint64_t *max1, const uint64_t *max2,
                    const float *cam1, const float *cam2, int n, const int32_t *triples, int H, int fix_scale, float *T12, float *R12,
                    float *t12, float *s12, int32_t *nin, uint8_t *flags, double *gap, float *err)
{
    int h, i, k;
    for (h = 0; h < H; h++) {
        float p1[9], p2[9], T21[16];
        const float *T = T12 + 16 * h;
        int cnt = 0;
        for (k = 0; k < 3; k++) {                                                        /* :172-173 */
            memcpy(p1 + 3 * k, X3Dc1 + 3 * triples[3 * h + k], sizeof(float) * 3);
            memcpy(p2 + 3 * k, X3Dc2 + 3 * triples[3 * h + k], sizeof(float) * 3);
        }
        s3o_compute_sim3(p1, p2, fix_scale, T12 + 16 * h, R12 + 9 * h, t12 + 3 * h, s12 + h, T21, NULL);
        for (i = 0; i < n; i++) {                                                        /* CheckInliers :340-364 */
            float a[2], b[2], d1[2], d2[2], err1, err2;
            double g = 1.0;
            int in;
            project(T, X3Dc2 + 3 * i, cam1, a);                                         /* vP2im1 */
            project(T21, X3Dc1 + 3 * i, cam2, b);                                       /* vP1im2 */
            d1[0] = P1im1[2 * i] - a[0]; d1[1] = P1im1[2 * i + 1] - a[1];
            d2[0] = b[0] - P2im2[2 * i]; d2[1] = b[1] - P2im2[2 * i + 1];
            err1 = (float)((double)d1[0] * d1[0] + (double)d1[1] * d1[1]);
            err2 = (float)((double)d2[0] * d2[0] + (double)d2[1] * d2[1]);
            in = s3o_is_inlier(err1, err2, max1[i], max2[i]);
            cnt += in;
            flags[(size_t)h * n + i] = (uint8_t)in;
            if (gap) { gap_cmp(&g, err1, (float)max1[i]); gap_cmp(&g, err2, (float)max2[i]); gap[(size_t)h * n + i] = g; }
            if (err) { err[2 * ((size_t)h * n + i)] = err1; err[2 * ((size_t)h * n + i) + 1] = err2; }
        }
        nin[h] = cnt;
    }
}

/* ------------------------------------------------------------------------------------------------ SetRansacParameters, iterate */
/* mRansacMaxIts of :120-137 for N correspondences.  ceil(..) -> int of a value no int holds (NaN when N = 0) is what x86's
 * cvttsd2si gives: INT_MIN */
int s3o_ransac_max_its(double probability, int minInliers, int maxIterations, int N)
{
    const float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N)
        nIterations = 1;
    else {
        const double v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
    }
    {
        const int lo = nIterations < maxIterations ? nIterations : maxIterations;
        return lo > 1 ? lo : 1;
    }
}

typedef struct s3o_fold {
    int32_t N, min_inliers, max_its;     /* set by the caller */
    int32_t iterations, best_inliers, best;   /* mnIterations, mnBestInliers, index of the hypothesis held as best (-1: none) */
} s3o_fold;

/* iterate(nIterations, bNoMore, ..) over counts[hypothesis index = mnIterations before the increment].  Returns the index of the
 * hypothesis whose T12 is returned, or -1 for the empty matrix; *nInliers as the reference sets it. */
int s3o_iterate(s3o_fold *f, const int32_t *counts, int nIterations, int *bNoMore, int *nInliers)
{
    int cur = 0;
    *bNoMore = 0; *nInliers = 0;
    if (f->N < f->min_inliers) { *bNoMore = 1; return -1; }                              /* :146 */
    while (f->iterations < f->max_its && cur < nIterations) {
        const int h = f->iterations;
        cur++; f->iterations++;
        if (counts[h] >= f->best_inliers) {                                              /* :183 */
            f->best_inliers = counts[h]; f->best = h;
            if (counts[h] > f->min_inliers) { *nInliers = counts[h]; return h; }         /* :192 */
        }
    }
    if (f->iterations >= f->max_its) *bNoMore = 1;                                       /* :203 */
    return -1;
}
