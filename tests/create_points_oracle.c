/* create_points_oracle.c -- CPU restatement of the per-pair arithmetic of LocalMapping::CreateNewMapPoints
 * (src/LocalMapping.cc:338-497) over flat arrays.  Test infrastructure: never part of the product.
 *
 * The search that feeds it (ORBmatcher::SearchForTriangulation) is oracle/match_oracle.c's literal function; the Python wrapper
 * (tests/create_points_oracle.py) runs the loop over the neighbours (:281-517) around the two.
 *
 * cv::Mat arithmetic (OpenCV 3.4, CV_32F; OpenCV is not available to this project, so parity with it is unpinned, like the other
 * OpenCV primitives of DESIGN section 5) is restated as:
 *   R * x            gemm's small-matrix case: the row sum a0 b0 + a1 b1 + a2 b2 in float, left to right
 *   R * x + t        ... then float(double(sum) + double(t))
 *   -R * t           ... float(double(sum) * -1.0)
 *   a.dot(b), norm   double sum of double products, left to right (norm: its sqrt)
 *   s * row - row    addWeighted with float weights: a * s + b * -1.0f in float
 *   v / s            convertTo with a FLOAT scale: v * float(1.0 / double(s))
 *   cv::SVD::compute JacobiSVDImpl_<float> (modules/core/src/lapack.cpp) on the transposed copy, eps = 2 FLT_EPSILON, at most 30 sweeps
 * cos / atan2 on float arguments are the float overloads (using namespace std): cosf / atan2f of the C library.
 *
 * Every comparison the reference evaluates on the way to a pair's status also records its GAP |lhs - rhs| / max(|lhs|, |rhs|);
 * the pair's gap is the smallest of them: a pair with a large gap keeps its status under last-bit differences of the arithmetic.
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -std=c99 -shared -fPIC. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { CPO_CREATED = 0, CPO_SKIPPED = 1, CPO_SVD_ZERO = 2, CPO_PARALLAX = 3, CPO_DEPTH = 4, CPO_REPROJ1 = 5, CPO_REPROJ2 = 6,
       CPO_DIST_ZERO = 7, CPO_SCALE = 8 };

typedef struct cpo_cam {
    float Tcw[16];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} cpo_cam;

typedef struct cpo_kp { float x, y, uright, depth; int32_t octave; } cpo_kp;

typedef struct cpo_result {
    int32_t status;
    int32_t from_svd;      /* x3d came out of the linear triangulation (A is valid) */
    int32_t sweeps;        /* Jacobi sweeps that applied a rotation, + 1 */
    float x3d[3];
    float A[16];
    double gap;
} cpo_result;

static void gap_cmp(double *gap, double lhs, double rhs)
{
    const double m = fmax(fabs(lhs), fabs(rhs));
    const double g = m > 0 ? fabs(lhs - rhs) / m : 0.0;
    if (g < *gap) *gap = g;
}

static float row3(const float *R, int r, float b0, float b1, float b2) { return R[3 * r] * b0 + R[3 * r + 1] * b1 + R[3 * r + 2] * b2; }
static float row3t(const float *R, int r, float b0, float b1, float b2, float t) { return (float)((double)row3(R, r, b0, b1, b2) + (double)t); }
static double dot3(const float *a, const float *b) { double s = 0; for (int k = 0; k < 3; ++k) s += (double)a[k] * (double)b[k]; return s; }
static double norm3(const float *a) { return sqrt(dot3(a, a)); }

/* Rcw, tcw, Rwc = Rcw.t(), Ow = -Rwc * tcw (KeyFrame::SetPose, src/KeyFrame.cc:69-85) of a 4 x 4 row-major Tcw */
void cpo_pose_parts(const float *Tcw, float *Rcw, float *tcw, float *Rwc, float *Ow)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { Rcw[3 * r + c] = Tcw[4 * r + c]; Rwc[3 * c + r] = Tcw[4 * r + c]; }
        tcw[r] = Tcw[4 * r + 3];
    }
    for (int r = 0; r < 3; ++r) Ow[r] = (float)((double)row3(Rwc, r, tcw[0], tcw[1], tcw[2]) * -1.0);
}

/* vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4 x 4 float A (row-major): JacobiSVDImpl_<float> on
 * At = A.t() (row i of At = column i of A), Vt = I; one-sided rotations of the row pairs until a sweep applies none. */
int cpo_svd_vt3(const float *A, float *v)
{
    float At[4][4], Vt[4][4];
    double W[4];
    const float eps = FLT_EPSILON * 2;
    int i, j, k, iter;
    for (i = 0; i < 4; ++i) {
        double sd = 0;
        for (k = 0; k < 4; ++k) { At[i][k] = A[4 * k + i]; const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sd;
        for (k = 0; k < 4; ++k) Vt[i][k] = 0;
        Vt[i][i] = 1;
    }
    for (iter = 0; iter < 30; ++iter) {
        int changed = 0;
        for (i = 0; i < 3; ++i)
            for (j = i + 1; j < 4; ++j) {
                float *Ai = At[i], *Aj = At[j];
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < 4; ++k) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt((double)a * b)) continue;
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
                for (k = 0; k < 4; ++k) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = 1;
                float *Vi = Vt[i], *Vj = Vt[j];
                for (k = 0; k < 4; ++k) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < 4; ++i) {
        double sd = 0;
        for (k = 0; k < 4; ++k) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (i = 0; i < 3; ++i) {       /* singular values descending, rows of Vt with them */
        j = i;
        for (k = i + 1; k < 4; ++k) if (W[j] < W[k]) j = k;
        if (i != j) {
            const double t = W[i]; W[i] = W[j]; W[j] = t;
            for (k = 0; k < 4; ++k) { const float u = Vt[i][k]; Vt[i][k] = Vt[j][k]; Vt[j][k] = u; }
        }
    }
    for (k = 0; k < 4; ++k) v[k] = Vt[3][k];
    return iter + 1;
}

/* One matched pair, src/LocalMapping.cc:338-497.  scale / sigma2 = mvScaleFactors / mvLevelSigma2 (one pyramid for the map). */
void cpo_pair(const cpo_cam *c1, const cpo_cam *c2, const cpo_kp *kp1, const cpo_kp *kp2, const float *scale, const float *sigma2,
              float scale_factor, cpo_result *out)
{
    float Rcw1[9], tcw1[3], Rwc1[9], Ow1[3], Rcw2[9], tcw2[3], Rwc2[9], Ow2[3];
    cpo_pose_parts(c1->Tcw, Rcw1, tcw1, Rwc1, Ow1);
    cpo_pose_parts(c2->Tcw, Rcw2, tcw2, Rwc2, Ow2);
    const float ratioFactor = 1.5f * scale_factor;                                      /* :276 */
    double gap = 1.0;
    memset(out, 0, sizeof(*out));
    const int bStereo1 = kp1->uright >= 0, bStereo2 = kp2->uright >= 0;                 /* :340, :344 */
    const float xn1[3] = {(kp1->x - c1->cx) * c1->invfx, (kp1->y - c1->cy) * c1->invfy, 1.0f};     /* :347-348 */
    const float xn2[3] = {(kp2->x - c2->cx) * c2->invfx, (kp2->y - c2->cy) * c2->invfy, 1.0f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; ++r) { ray1[r] = row3(Rwc1, r, xn1[0], xn1[1], xn1[2]); ray2[r] = row3(Rwc2, r, xn2[0], xn2[1], xn2[2]); }
    const float cosParallaxRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));         /* :352 */
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = cosf(2 * atan2f(c1->mb / 2, kp1->depth));         /* :358-361 */
    else if (bStereo2) cosParallaxStereo2 = cosf(2 * atan2f(c2->mb / 2, kp2->depth));
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   /* std::min(a, b): b < a ? b : a */

    float x3D[3];
    int linear = 0;
    /* :366 with its short circuits */
    gap_cmp(&gap, cosParallaxRays, cosParallaxStereo);
    if (cosParallaxRays < cosParallaxStereo) {
        gap_cmp(&gap, cosParallaxRays, 0.0);
        if (cosParallaxRays > 0) {
            if (bStereo1 || bStereo2) linear = 1;
            else { gap_cmp(&gap, (double)cosParallaxRays, 0.9997); linear = (double)cosParallaxRays < 0.9997; }
        }
    }
    if (linear) {
        float *A = out->A, v[4];                                                            /* :369-373 */
        for (int c = 0; c < 4; ++c) {
            A[c] = xn1[0] * c1->Tcw[8 + c] + c1->Tcw[c] * -1.0f;
            A[4 + c] = xn1[1] * c1->Tcw[8 + c] + c1->Tcw[4 + c] * -1.0f;
            A[8 + c] = xn2[0] * c2->Tcw[8 + c] + c2->Tcw[c] * -1.0f;
            A[12 + c] = xn2[1] * c2->Tcw[8 + c] + c2->Tcw[4 + c] * -1.0f;
        }
        out->sweeps = cpo_svd_vt3(A, v);
        out->from_svd = 1;
        if (v[3] == 0) { out->status = CPO_SVD_ZERO; out->gap = 0.0; return; }              /* :380 */
        const float inv = (float)(1.0 / (double)v[3]);                                     /* :387 */
        for (int r = 0; r < 3; ++r) x3D[r] = v[r] * inv;
    } else {
        int side = 0;
        if (bStereo1) { gap_cmp(&gap, cosParallaxStereo1, cosParallaxStereo2); if (cosParallaxStereo1 < cosParallaxStereo2) side = 1; }
        if (!side && bStereo2) { gap_cmp(&gap, cosParallaxStereo2, cosParallaxStereo1); if (cosParallaxStereo2 < cosParallaxStereo1) side = 2; }
        if (!side) { out->status = CPO_PARALLAX; out->gap = gap; return; }                  /* :398-402 */
        const cpo_cam *c = side == 1 ? c1 : c2;                                            /* KeyFrame::UnprojectStereo, src/KeyFrame.cc:659-675 */
        const cpo_kp *kp = side == 1 ? kp1 : kp2;
        const float z = kp->depth;
        if (!(z > 0)) { out->status = CPO_PARALLAX; out->gap = 0.0; return; }               /* (the reference returns an empty Mat and fails) */
        const float x = (kp->x - c->cx) * z * c->invfx, y = (kp->y - c->cy) * z * c->invfy;
        for (int r = 0; r < 3; ++r) x3D[r] = row3t(side == 1 ? Rwc1 : Rwc2, r, x, y, z, (side == 1 ? Ow1 : Ow2)[r]);
    }
    memcpy(out->x3d, x3D, sizeof(x3D));

    const double d1z = dot3(Rcw1 + 6, x3D);
    const float z1 = (float)(d1z + (double)tcw1[2]);                                       /* :407 */
    gap_cmp(&gap, d1z, -(double)tcw1[2]);
    if (z1 <= 0) { out->status = CPO_DEPTH; out->gap = gap; return; }
    const double d2z = dot3(Rcw2 + 6, x3D);
    const float z2 = (float)(d2z + (double)tcw2[2]);                                       /* :414 */
    gap_cmp(&gap, d2z, -(double)tcw2[2]);
    if (z2 <= 0) { out->status = CPO_DEPTH; out->gap = gap; return; }

    {   /* :421-452 */
        const float sigmaSquare1 = sigma2[kp1->octave];
        const float x1 = (float)(dot3(Rcw1, x3D) + (double)tcw1[0]), y1 = (float)(dot3(Rcw1 + 3, x3D) + (double)tcw1[1]);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = c1->fx * x1 * invz1 + c1->cx, v1 = c1->fy * y1 * invz1 + c1->cy;
        const float errX1 = u1 - kp1->x, errY1 = v1 - kp1->y;
        double lhs, rhs;
        if (!bStereo1) { lhs = (double)(errX1 * errX1 + errY1 * errY1); rhs = 5.991 * (double)sigmaSquare1; }
        else {
            const float u1_r = u1 - c1->mbf * invz1, errX1_r = u1_r - kp1->uright;
            lhs = (double)(errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r); rhs = 7.8 * (double)sigmaSquare1;
        }
        gap_cmp(&gap, lhs, rhs);
        if (lhs > rhs) { out->status = CPO_REPROJ1; out->gap = gap; return; }
    }
    {   /* :454-478; :471 takes the CURRENT keyframe's mbf */
        const float sigmaSquare2 = sigma2[kp2->octave];
        const float x2 = (float)(dot3(Rcw2, x3D) + (double)tcw2[0]), y2 = (float)(dot3(Rcw2 + 3, x3D) + (double)tcw2[1]);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = c2->fx * x2 * invz2 + c2->cx, v2 = c2->fy * y2 * invz2 + c2->cy;
        const float errX2 = u2 - kp2->x, errY2 = v2 - kp2->y;
        double lhs, rhs;
        if (!bStereo2) { lhs = (double)(errX2 * errX2 + errY2 * errY2); rhs = 5.991 * (double)sigmaSquare2; }
        else {
            const float u2_r = u2 - c1->mbf * invz2, errX2_r = u2_r - kp2->uright;
            lhs = (double)(errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r); rhs = 7.8 * (double)sigmaSquare2;
        }
        gap_cmp(&gap, lhs, rhs);
        if (lhs > rhs) { out->status = CPO_REPROJ2; out->gap = gap; return; }
    }
    {   /* :480-497 */
        const float n1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]}, n2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
        const float dist1 = (float)norm3(n1), dist2 = (float)norm3(n2);
        if (dist1 == 0 || dist2 == 0) { out->status = CPO_DIST_ZERO; out->gap = 0.0; return; }
        const float ratioDist = dist2 / dist1;
        const float ratioOctave = scale[kp1->octave] / scale[kp2->octave];
        gap_cmp(&gap, ratioDist * ratioFactor, ratioOctave);
        if (ratioDist * ratioFactor < ratioOctave) { out->status = CPO_SCALE; out->gap = gap; return; }
        gap_cmp(&gap, ratioDist, ratioOctave * ratioFactor);
        if (ratioDist > ratioOctave * ratioFactor) { out->status = CPO_SCALE; out->gap = gap; return; }
    }
    out->status = CPO_CREATED;
    out->gap = gap;
}

void cpo_pairs(const cpo_cam *c1, const cpo_cam *c2, const cpo_kp *kps1, const cpo_kp *kps2, const int32_t *idx1, const int32_t *idx2,
               int npairs, const float *scale, const float *sigma2, float scale_factor, cpo_result *out)
{
    for (int p = 0; p < npairs; ++p) cpo_pair(c1, c2, kps1 + idx1[p], kps2 + idx2[p], scale, sigma2, scale_factor, out + p);
}
