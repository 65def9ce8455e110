/* pnp_oracle.c -- a literal CPU restatement of PnPsolver (src/PnPsolver.cc): EPnP (:831-1457) with the arrays the reference keeps
 * (pws, us, alphas, pcs, the 2n x 12 matrix M), CheckInliers (:763-794), Refine (:649-694), SetRansacParameters (:123-159), the fold
 * of the original iterate (:170-263) and of the first stage of iterate(Frame &, .., Map *) (:267-416).  Test infrastructure: never
 * part of the product, and written from the reference's lines, not from orb_slam2_e_amd/csrc/orbm_epnp.h.
 *
 * The OpenCV primitives are restated from OpenCV 3.4 in their general run-time form (unpinned): cvMulTransposed(.., 1),
 * JacobiSVDImpl_<double> behind cvSVD / cvInvert(CV_SVD) / cvSolve(CV_SVD), SVBkSb.  The SVD's hypot is pno_hypot: OpenCV's own
 * JacobiImpl_ form by default (the product's stated departure), libm's with -DPNP_LIBM_HYPOT (what the reference links).
 * gauss_newton's x[4], indeterminate in the reference when qr_solve returns early in the first iteration, starts as 0. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static double pno_hypot(double a, double b)
{
#ifdef PNP_LIBM_HYPOT
    return hypot(a, b);
#else
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
#endif
}

static unsigned rng_next(uint64_t *state)
{
    *state = (uint64_t)(unsigned)*state * 4164903690U + (unsigned)(*state >> 32);
    return (unsigned)*state;
}

/* JacobiSVDImpl_<double>: At n1 rows (the first n meaningful) of length m with row stride astep, Vt n x n (may be NULL) */
static int jacobi_svd(double *At, int astep, double *_W, double *Vt, int vstep, int m, int n, int n1)
{
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    double *W = (double *)malloc(sizeof(double) * (size_t)n);
    int i, j, k, iter, max_iter = m > 30 ? m : 30, rotations = 0;
    double c, s, sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { double t = At[i * astep + k]; sd += t * t; }
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
                double *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = pno_hypot(p, beta);
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    double t0 = c * Ai[k] + s * Aj[k];
                    double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = 1; rotations++;
                if (Vt) {
                    double *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                    for (k = 0; k < n; k++) {
                        double t0 = c * Vi[k] + s * Vj[k];
                        double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { double t = At[i * astep + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double t = W[i]; W[i] = W[j]; W[j] = t;
            if (Vt) {
                for (k = 0; k < m; k++) { t = At[i * astep + k]; At[i * astep + k] = At[j * astep + k]; At[j * astep + k] = t; }
                for (k = 0; k < n; k++) { t = Vt[i * vstep + k]; Vt[i * vstep + k] = Vt[j * vstep + k]; Vt[j * vstep + k] = t; }
            }
        }
    }
    for (i = 0; i < n; i++) _W[i] = W[i];
    if (Vt) {
        uint64_t rng = 0x12345678;
        for (i = 0; i < n1; i++) {
            sd = i < n ? W[i] : 0;
            for (int ii = 0; ii < 100 && sd <= minval; ii++) {
                const double val0 = 1. / m;
                for (k = 0; k < m; k++) At[i * astep + k] = (rng_next(&rng) & 256) != 0 ? val0 : -val0;
                for (iter = 0; iter < 2; iter++)
                    for (j = 0; j < i; j++) {
                        sd = 0;
                        for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                        double asum = 0;
                        for (k = 0; k < m; k++) {
                            double t = At[i * astep + k] - sd * At[j * astep + k];
                            At[i * astep + k] = t;
                            asum += fabs(t);
                        }
                        asum = asum > eps * 100 ? 1 / asum : 0;
                        for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                    }
                sd = 0;
                for (k = 0; k < m; k++) { double t = At[i * astep + k]; sd += t * t; }
                sd = sqrt(sd);
            }
            s = sd > minval ? 1 / sd : 0.;
            for (k = 0; k < m; k++) At[i * astep + k] *= s;
        }
    }
    free(W);
    return rotations;
}

/* _SVDcompute for a rows x cols double matrix, rows >= cols, without FULL_UV: w [cols], u [rows][cols] (may be NULL),
 * vt [cols][cols] (may be NULL); V is computed whenever either is asked for */
static void svd_compute(const double *src, int rows, int cols, double *w, double *u, double *vt)
{
    const int m = rows, n = cols;
    double *temp_a = (double *)malloc(sizeof(double) * (size_t)(n * m)), *temp_v = (double *)malloc(sizeof(double) * (size_t)(n * n));
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) temp_a[i * m + k] = src[k * n + i];
    jacobi_svd(temp_a, m, w, (u || vt) ? temp_v : NULL, n, m, n, n);
    if (u)
        for (int k = 0; k < m; k++)
            for (int i = 0; i < n; i++) u[k * n + i] = temp_a[i * m + k];
    if (vt) memcpy(vt, temp_v, sizeof(double) * (size_t)(n * n));
    free(temp_a); free(temp_v);
}

/* cvSVD(A, W, U, V, flags) of a square n x n matrix: ut != 0: U comes transposed (CV_SVD_U_T); V (may be NULL) comes untransposed */
static void cv_svd_square(const double *A, int n, double *W, double *U, int u_t, double *V)
{
    double *u = (double *)malloc(sizeof(double) * (size_t)(n * n)), *vt = (double *)malloc(sizeof(double) * (size_t)(n * n));
    svd_compute(A, n, n, W, u, V ? vt : NULL);
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) U[r * n + c] = u_t ? u[c * n + r] : u[r * n + c];
    if (V)
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) V[r * n + c] = vt[c * n + r];
    free(u); free(vt);
}

/* SVBkSbImpl_<double> with nb == 1 and a right-hand side, or without one (b == NULL: nb = m) */
static void sv_bk_sb(int m, int n, const double *w, const double *u, int ldu, int uT, const double *v, int ldv, int vT, const double *b, double *x,
                     int ldx)
{
    double threshold = 0;
    const int udelta0 = uT ? ldu : 1, udelta1 = uT ? 1 : ldu, vdelta0 = vT ? ldv : 1, vdelta1 = vT ? 1 : ldv;
    const int nm = m < n ? m : n, nb = b ? 1 : m;
    int i, j;
    for (i = 0; i < n; i++)
        for (j = 0; j < nb; j++) x[i * ldx + j] = 0;
    for (i = 0; i < nm; i++) threshold += w[i];
    threshold *= DBL_EPSILON * 2;
    for (i = 0; i < nm; i++, u += udelta0, v += vdelta0) {
        double wi = w[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (nb == 1) {
            double s = 0;
            if (b)
                for (j = 0; j < m; j++) s += u[j * udelta1] * b[j];
            else
                s = u[0];
            s *= wi;
            for (j = 0; j < n; j++) x[j * ldx] = x[j * ldx] + s * v[j * vdelta1];
        } else {
            double buffer[16];
            for (j = 0; j < nb; j++) buffer[j] = u[j * udelta1] * wi;
            for (int r = 0; r < n; r++) {                      /* MatrAXPY(n, nb, buffer, 0, v, vdelta1, x, ldx) */
                const double s = v[r * vdelta1];
                for (j = 0; j < nb; j++) x[r * ldx + j] = x[r * ldx + j] + s * buffer[j];
            }
        }
    }
}

/* cvSolve(A, b, x, CV_SVD): A m x n (m >= n), b m x 1 */
void pno_solve_svd(const double *A, int m, int n, const double *b, double *x)
{
    double *a = (double *)malloc(sizeof(double) * (size_t)(n * m)), *v = (double *)malloc(sizeof(double) * (size_t)(n * n)), w[16];
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) a[i * m + k] = A[k * n + i];
    jacobi_svd(a, m, w, v, n, m, n, n);
    sv_bk_sb(m, n, w, a, m, 1, v, n, 1, b, x, 1);
    free(a); free(v);
}

/* cvInvert(A, Ainv, CV_SVD), n x n (n <= 16) */
void pno_invert_svd(const double *A, int n, double *inv)
{
    double *u = (double *)malloc(sizeof(double) * (size_t)(n * n)), *vt = (double *)malloc(sizeof(double) * (size_t)(n * n)), w[16];
    svd_compute(A, n, n, w, u, vt);
    sv_bk_sb(n, n, w, u, n, 0, vt, n, 1, NULL, inv, n);
    free(u); free(vt);
}

/* cvSVD(A, W, Ut, 0, MODIFY_A | U_T) of a square matrix (test entry) */
void pno_svd_ut(const double *A, int n, double *W, double *Ut) { cv_svd_square(A, n, W, Ut, 1, NULL); }

/* cvMulTransposed(src, dst, 1): dst = src.t() * src, src rows x cols */
static void mul_transposed(const double *src, int rows, int cols, double *dst)
{
    for (int i = 0; i < cols; i++)
        for (int j = i; j < cols; j++) {
            double s0 = 0;
            for (int k = 0; k < rows; k++) s0 += src[k * cols + i] * src[k * cols + j];
            dst[i * cols + j] = s0;
        }
    for (int i = 1; i < cols; i++)
        for (int j = 0; j < i; j++) dst[i * cols + j] = dst[j * cols + i];
}

/* ------------------------------------------------------------------------------------------------ the epnp members */
typedef struct {
    double uc, vc, fu, fv;
    double *pws, *us, *alphas, *pcs;
    int number_of_correspondences;
    double cws[4][3], ccs[4][3];
    int singular;                   /* qr_solve's early returns in the last compute_pose */
} epnp;

static double dot(const double *v1, const double *v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }
static double dist2(const double *p1, const double *p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

static void choose_control_points(epnp *e)
{
    const int n = e->number_of_correspondences;
    e->cws[0][0] = e->cws[0][1] = e->cws[0][2] = 0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) e->cws[0][j] += e->pws[3 * i + j];
    for (int j = 0; j < 3; j++) e->cws[0][j] /= n;
    double *PW0 = (double *)malloc(sizeof(double) * 3 * (size_t)n);
    double pw0tpw0[9], dc[3], uct[9];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) PW0[3 * i + j] = e->pws[3 * i + j] - e->cws[0][j];
    mul_transposed(PW0, n, 3, pw0tpw0);
    cv_svd_square(pw0tpw0, 3, dc, uct, 1, NULL);
    free(PW0);
    for (int i = 1; i < 4; i++) {
        double k = sqrt(dc[i - 1] / n);
        for (int j = 0; j < 3; j++) e->cws[i][j] = e->cws[0][j] + k * uct[3 * (i - 1) + j];
    }
}

static void compute_barycentric_coordinates(epnp *e)
{
    double cc[9], cc_inv[9];
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = e->cws[j][i] - e->cws[0][i];
    pno_invert_svd(cc, 3, cc_inv);
    double *ci = cc_inv;
    for (int i = 0; i < e->number_of_correspondences; i++) {
        double *pi = e->pws + 3 * i;
        double *a = e->alphas + 4 * i;
        for (int j = 0; j < 3; j++)
            a[1 + j] = ci[3 * j] * (pi[0] - e->cws[0][0]) + ci[3 * j + 1] * (pi[1] - e->cws[0][1]) + ci[3 * j + 2] * (pi[2] - e->cws[0][2]);
        a[0] = 1.0f - a[1] - a[2] - a[3];
    }
}

static void fill_M(const epnp *e, double *M, const int row, const double *as, const double u, const double v)
{
    double *M1 = M + row * 12;
    double *M2 = M1 + 12;
    for (int i = 0; i < 4; i++) {
        M1[3 * i] = as[i] * e->fu;
        M1[3 * i + 1] = 0.0;
        M1[3 * i + 2] = as[i] * (e->uc - u);
        M2[3 * i] = 0.0;
        M2[3 * i + 1] = as[i] * e->fv;
        M2[3 * i + 2] = as[i] * (e->vc - v);
    }
}

static void compute_ccs(epnp *e, const double *betas, const double *ut)
{
    for (int i = 0; i < 4; i++) e->ccs[i][0] = e->ccs[i][1] = e->ccs[i][2] = 0.0f;
    for (int i = 0; i < 4; i++) {
        const double *v = ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) e->ccs[j][k] += betas[i] * v[3 * j + k];
    }
}

static void compute_pcs(epnp *e)
{
    for (int i = 0; i < e->number_of_correspondences; i++) {
        double *a = e->alphas + 4 * i;
        double *pc = e->pcs + 3 * i;
        for (int j = 0; j < 3; j++) pc[j] = a[0] * e->ccs[0][j] + a[1] * e->ccs[1][j] + a[2] * e->ccs[2][j] + a[3] * e->ccs[3][j];
    }
}

static void solve_for_sign(epnp *e)
{
    if (e->pcs[2] < 0.0) {
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 3; j++) e->ccs[i][j] = -e->ccs[i][j];
        for (int i = 0; i < e->number_of_correspondences; i++) {
            e->pcs[3 * i] = -e->pcs[3 * i];
            e->pcs[3 * i + 1] = -e->pcs[3 * i + 1];
            e->pcs[3 * i + 2] = -e->pcs[3 * i + 2];
        }
    }
}

static double reprojection_error(const epnp *e, double R[3][3], const double t[3])
{
    double sum2 = 0.0;
    for (int i = 0; i < e->number_of_correspondences; i++) {
        double *pw = e->pws + 3 * i;
        double Xc = dot(R[0], pw) + t[0];
        double Yc = dot(R[1], pw) + t[1];
        double inv_Zc = 1.0 / (dot(R[2], pw) + t[2]);
        double ue = e->uc + e->fu * Xc * inv_Zc;
        double ve = e->vc + e->fv * Yc * inv_Zc;
        double u = e->us[2 * i], v = e->us[2 * i + 1];
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / e->number_of_correspondences;
}

static void estimate_R_and_t(epnp *e, double R[3][3], double t[3])
{
    const int n = e->number_of_correspondences;
    double pc0[3], pw0[3];
    pc0[0] = pc0[1] = pc0[2] = 0.0;
    pw0[0] = pw0[1] = pw0[2] = 0.0;
    for (int i = 0; i < n; i++) {
        const double *pc = e->pcs + 3 * i;
        const double *pw = e->pws + 3 * i;
        for (int j = 0; j < 3; j++) { pc0[j] += pc[j]; pw0[j] += pw[j]; }
    }
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9], abt_d[3], abt_u[9], abt_v[9];
    memset(abt, 0, sizeof(abt));
    for (int i = 0; i < n; i++) {
        double *pc = e->pcs + 3 * i;
        double *pw = e->pws + 3 * i;
        for (int j = 0; j < 3; j++) {
            abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
            abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
            abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
    }
    cv_svd_square(abt, 3, abt_d, abt_u, 0, abt_v);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = dot(abt_u + 3 * i, abt_v + 3 * j);
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
                       R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) {
        R[2][0] = -R[2][0];
        R[2][1] = -R[2][1];
        R[2][2] = -R[2][2];
    }
    t[0] = pc0[0] - dot(R[0], pw0);
    t[1] = pc0[1] - dot(R[1], pw0);
    t[2] = pc0[2] - dot(R[2], pw0);
}

static double compute_R_and_t(epnp *e, const double *ut, const double *betas, double R[3][3], double t[3])
{
    compute_ccs(e, betas, ut);
    compute_pcs(e);
    solve_for_sign(e);
    estimate_R_and_t(e, R, t);
    return reprojection_error(e, R, t);
}

static void find_betas_approx_1(const double *l_6x10, const double *rho, double *betas)
{
    double l_6x4[6 * 4], b4[4];
    for (int i = 0; i < 6; i++) {
        l_6x4[4 * i] = l_6x10[10 * i];
        l_6x4[4 * i + 1] = l_6x10[10 * i + 1];
        l_6x4[4 * i + 2] = l_6x10[10 * i + 3];
        l_6x4[4 * i + 3] = l_6x10[10 * i + 6];
    }
    pno_solve_svd(l_6x4, 6, 4, rho, b4);
    if (b4[0] < 0) {
        betas[0] = sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0];
        betas[2] = -b4[2] / betas[0];
        betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = sqrt(b4[0]);
        betas[1] = b4[1] / betas[0];
        betas[2] = b4[2] / betas[0];
        betas[3] = b4[3] / betas[0];
    }
}

static void find_betas_approx_2(const double *l_6x10, const double *rho, double *betas)
{
    double l_6x3[6 * 3], b3[3];
    for (int i = 0; i < 6; i++) {
        l_6x3[3 * i] = l_6x10[10 * i];
        l_6x3[3 * i + 1] = l_6x10[10 * i + 1];
        l_6x3[3 * i + 2] = l_6x10[10 * i + 2];
    }
    pno_solve_svd(l_6x3, 6, 3, rho, b3);
    if (b3[0] < 0) {
        betas[0] = sqrt(-b3[0]);
        betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
        betas[0] = sqrt(b3[0]);
        betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) betas[0] = -betas[0];
    betas[2] = 0.0;
    betas[3] = 0.0;
}

static void find_betas_approx_3(const double *l_6x10, const double *rho, double *betas)
{
    double l_6x5[6 * 5], b5[5];
    for (int i = 0; i < 6; i++)
        for (int c = 0; c < 5; c++) l_6x5[5 * i + c] = l_6x10[10 * i + c];
    pno_solve_svd(l_6x5, 6, 5, rho, b5);
    if (b5[0] < 0) {
        betas[0] = sqrt(-b5[0]);
        betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
        betas[0] = sqrt(b5[0]);
        betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) betas[0] = -betas[0];
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
}

static void compute_L_6x10(const double *ut, double *l_6x10)
{
    const double *v[4];
    v[0] = ut + 12 * 11;
    v[1] = ut + 12 * 10;
    v[2] = ut + 12 * 9;
    v[3] = ut + 12 * 8;
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
            dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
            dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double *row = l_6x10 + 10 * i;
        row[0] = dot(dv[0][i], dv[0][i]);
        row[1] = 2.0f * dot(dv[0][i], dv[1][i]);
        row[2] = dot(dv[1][i], dv[1][i]);
        row[3] = 2.0f * dot(dv[0][i], dv[2][i]);
        row[4] = 2.0f * dot(dv[1][i], dv[2][i]);
        row[5] = dot(dv[2][i], dv[2][i]);
        row[6] = 2.0f * dot(dv[0][i], dv[3][i]);
        row[7] = 2.0f * dot(dv[1][i], dv[3][i]);
        row[8] = 2.0f * dot(dv[2][i], dv[3][i]);
        row[9] = dot(dv[3][i], dv[3][i]);
    }
}

static void compute_rho(const epnp *e, double *rho)
{
    rho[0] = dist2(e->cws[0], e->cws[1]);
    rho[1] = dist2(e->cws[0], e->cws[2]);
    rho[2] = dist2(e->cws[0], e->cws[3]);
    rho[3] = dist2(e->cws[1], e->cws[2]);
    rho[4] = dist2(e->cws[1], e->cws[3]);
    rho[5] = dist2(e->cws[2], e->cws[3]);
}

static void compute_A_and_b_gauss_newton(const double *l_6x10, const double *rho, double betas[4], double *A, double *b)
{
    for (int i = 0; i < 6; i++) {
        const double *rowL = l_6x10 + i * 10;
        double *rowA = A + i * 4;
        rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
        rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
        rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
        rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
        b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                         rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                         rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                         rowL[9] * betas[3] * betas[3]);
    }
}

/* qr_solve with the reference's pointer walk; returns 0 on its "A is singular" early return */
static int qr_solve(double *pA, int nr, int nc, double *pb, double *pX)
{
    double A1[8], A2[8];
    double *ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double *ppAik = ppAkk, eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {
            double elt = fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return 0;
        } else {
            double *ppAik = ppAkk, sum = 0.0, inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) {
                *ppAik *= inv_eta;
                sum += *ppAik * *ppAik;
                ppAik += nc;
            }
            double sigma = sqrt(sum);
            if (*ppAkk < 0) sigma = -sigma;
            *ppAkk += sigma;
            A1[k] = sigma * *ppAkk;
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                double *ppAik = ppAkk, sum = 0;
                for (int i = k; i < nr; i++) {
                    sum += *ppAik * ppAik[j - k];
                    ppAik += nc;
                }
                double tau = sum / A1[k];
                ppAik = ppAkk;
                for (int i = k; i < nr; i++) {
                    ppAik[j - k] -= tau * *ppAik;
                    ppAik += nc;
                }
            }
        }
        ppAkk += nc + 1;
    }
    double *ppAjj = pA;
    for (int j = 0; j < nc; j++) {
        double *ppAij = ppAjj, tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double *ppAij = pA + i * nc + (i + 1), sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
    return 1;
}

static void gauss_newton(epnp *e, const double *l_6x10, const double *rho, double betas[4])
{
    const int iterations_number = 5;
    double a[6 * 4], b[6], x[4] = {0, 0, 0, 0};
    for (int k = 0; k < iterations_number; k++) {
        compute_A_and_b_gauss_newton(l_6x10, rho, betas, a, b);
        if (!qr_solve(a, 6, 4, b, x)) e->singular++;
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

static double compute_pose(epnp *e, double R[3][3], double t[3])
{
    const int n = e->number_of_correspondences;
    e->singular = 0;
    choose_control_points(e);
    compute_barycentric_coordinates(e);
    double *M = (double *)malloc(sizeof(double) * 24 * (size_t)n);
    for (int i = 0; i < n; i++) fill_M(e, M, 2 * i, e->alphas + 4 * i, e->us[2 * i], e->us[2 * i + 1]);
    double mtm[12 * 12], d[12], ut[12 * 12];
    mul_transposed(M, 2 * n, 12, mtm);
    cv_svd_square(mtm, 12, d, ut, 1, NULL);
    free(M);
    double l_6x10[6 * 10], rho[6];
    compute_L_6x10(ut, l_6x10);
    compute_rho(e, rho);
    double Betas[4][4], rep_errors[4];
    double Rs[4][3][3], ts[4][3];
    find_betas_approx_1(l_6x10, rho, Betas[1]);
    gauss_newton(e, l_6x10, rho, Betas[1]);
    rep_errors[1] = compute_R_and_t(e, ut, Betas[1], Rs[1], ts[1]);
    find_betas_approx_2(l_6x10, rho, Betas[2]);
    gauss_newton(e, l_6x10, rho, Betas[2]);
    rep_errors[2] = compute_R_and_t(e, ut, Betas[2], Rs[2], ts[2]);
    find_betas_approx_3(l_6x10, rho, Betas[3]);
    gauss_newton(e, l_6x10, rho, Betas[3]);
    rep_errors[3] = compute_R_and_t(e, ut, Betas[3], Rs[3], ts[3]);
    int N = 1;
    if (rep_errors[2] < rep_errors[1]) N = 2;
    if (rep_errors[3] < rep_errors[N]) N = 3;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = Rs[N][i][j];
        t[i] = ts[N][i];
    }
    return rep_errors[N];
}

static void epnp_alloc(epnp *e, int n, const double *cam)
{
    e->fu = cam[0]; e->fv = cam[1]; e->uc = cam[2]; e->vc = cam[3];
    e->pws = (double *)malloc(sizeof(double) * 3 * (size_t)n); e->us = (double *)malloc(sizeof(double) * 2 * (size_t)n);
    e->alphas = (double *)malloc(sizeof(double) * 4 * (size_t)n); e->pcs = (double *)malloc(sizeof(double) * 3 * (size_t)n);
    e->number_of_correspondences = 0;
}
static void epnp_free(epnp *e) { free(e->pws); free(e->us); free(e->alphas); free(e->pcs); }
static void add_correspondence(epnp *e, double X, double Y, double Z, double u, double v)
{
    const int k = e->number_of_correspondences;
    e->pws[3 * k] = X; e->pws[3 * k + 1] = Y; e->pws[3 * k + 2] = Z;
    e->us[2 * k] = u; e->us[2 * k + 1] = v;
    e->number_of_correspondences++;
}

/* compute_pose of n correspondences given in double; returns the number of qr_solve early returns */
int pno_pose(const double *pws, const double *us, int n, const double *cam, double *R, double *t, double *rep_error)
{
    epnp e;
    double Rm[3][3];
    epnp_alloc(&e, n, cam);
    for (int i = 0; i < n; i++) add_correspondence(&e, pws[3 * i], pws[3 * i + 1], pws[3 * i + 2], us[2 * i], us[2 * i + 1]);
    *rep_error = compute_pose(&e, Rm, t);
    memcpy(R, Rm, sizeof(Rm));
    epnp_free(&e);
    return e.singular;
}

/* CheckInliers (:763-794): flags [n], returns mnInliersi */
static int check_inliers(double mRi[3][3], const double mti[3], const float *mvP3Dw, const float *mvP2D, const float *mvMaxError, int N, const double *cam,
                         uint8_t *mvbInliersi)
{
    const double fu = cam[0], fv = cam[1], uc = cam[2], vc = cam[3];
    int mnInliersi = 0;
    for (int i = 0; i < N; i++) {
        const float *P3Dw = mvP3Dw + 3 * i, *P2D = mvP2D + 2 * i;
        float Xc = mRi[0][0] * P3Dw[0] + mRi[0][1] * P3Dw[1] + mRi[0][2] * P3Dw[2] + mti[0];
        float Yc = mRi[1][0] * P3Dw[0] + mRi[1][1] * P3Dw[1] + mRi[1][2] * P3Dw[2] + mti[1];
        float invZc = 1 / (mRi[2][0] * P3Dw[0] + mRi[2][1] * P3Dw[1] + mRi[2][2] * P3Dw[2] + mti[2]);
        double ue = uc + fu * Xc * invZc;
        double ve = vc + fv * Yc * invZc;
        float distX = P2D[0] - ue;
        float distY = P2D[1] - ve;
        float error2 = distX * distX + distY * distY;
        if (error2 < mvMaxError[i]) {
            mvbInliersi[i] = 1;
            mnInliersi++;
        } else
            mvbInliersi[i] = 0;
    }
    return mnInliersi;
}

int pno_check_inliers(const double *R, const double *t, const float *X, const float *uv, const float *max_error, int N, const double *cam, uint8_t *flags)
{
    double Rm[3][3];
    memcpy(Rm, R, sizeof(Rm));
    return check_inliers(Rm, t, X, uv, max_error, N, cam, flags);
}

/* Refine (:649-694) on the flags `best`: pose, refined flags, returns mnRefinedInliers */
int pno_refine(const float *X, const float *uv, const float *max_error, int N, const double *cam, const uint8_t *best, double *R, double *t,
               uint8_t *refined)
{
    epnp e;
    double Rm[3][3];
    int cnt = 0;
    for (int i = 0; i < N; i++) cnt += best[i] != 0;
    epnp_alloc(&e, cnt ? cnt : 1, cam);
    for (int i = 0; i < N; i++)
        if (best[i]) add_correspondence(&e, X[3 * i], X[3 * i + 1], X[3 * i + 2], uv[2 * i], uv[2 * i + 1]);
    compute_pose(&e, Rm, t);
    memcpy(R, Rm, sizeof(Rm));
    epnp_free(&e);
    return check_inliers(Rm, t, X, uv, max_error, N, cam, refined);
}

/* What orbm_pnp_hypotheses computes for one problem: per set compute_pose + CheckInliers, then in order the records (count >=
 * min_inliers and > the running best, which starts at best_in) and Refine on each record's flags.  Outputs by hypothesis; the
 * refined ones are 0 where refined[h] == 0.  singular [H] (may be NULL): qr_solve early returns of the hypothesis. */
void pno_problem(const float *X, const float *uv, const int32_t *octave, const int32_t *sets, int n, int H, const double *cam, float th2,
                 const float *sigma2, int min_inliers, int best_in, double *R, double *t, double *rep, int32_t *nin, int32_t *refined, double *Rr,
                 double *tr, int32_t *nref, uint8_t *flags, uint8_t *rflags, int32_t *singular)
{
    float *max_error = (float *)malloc(sizeof(float) * (size_t)(n ? n : 1));
    for (int i = 0; i < n; i++) max_error[i] = sigma2[octave[i]] * th2;           /* :157-158 */
    int best = best_in;
    for (int h = 0; h < H; h++) {
        epnp e;
        double Rm[3][3];
        epnp_alloc(&e, 4, cam);
        for (int k = 0; k < 4; k++) {
            const int idx = sets[4 * h + k];
            add_correspondence(&e, X[3 * idx], X[3 * idx + 1], X[3 * idx + 2], uv[2 * idx], uv[2 * idx + 1]);
        }
        rep[h] = compute_pose(&e, Rm, t + 3 * h);
        if (singular) singular[h] = e.singular;
        epnp_free(&e);
        memcpy(R + 9 * h, Rm, sizeof(Rm));
        nin[h] = check_inliers(Rm, t + 3 * h, X, uv, max_error, n, cam, flags + (size_t)h * n);
        refined[h] = 0; nref[h] = 0;
        memset(Rr + 9 * h, 0, sizeof(double) * 9); memset(tr + 3 * h, 0, sizeof(double) * 3); memset(rflags + (size_t)h * n, 0, (size_t)n);
        if (nin[h] >= min_inliers && nin[h] > best) {
            best = nin[h];
            refined[h] = 1;
            nref[h] = pno_refine(X, uv, max_error, n, cam, flags + (size_t)h * n, Rr + 9 * h, tr + 3 * h, rflags + (size_t)h * n);
        }
    }
    free(max_error);
}

/* SetRansacParameters (:123-159) */
typedef struct {
    int32_t N, min_inliers, max_its, iterations, best_inliers, best;   /* mRansacMinInliers, mRansacMaxIts, mnIterations, mnBestInliers, its hypothesis */
    float epsilon;
    int32_t last_refined;          /* mnRefinedInliers of the last Refine() */
} pno_fold;

void pno_set_ransac_parameters(pno_fold *f, double probability, int minInliers, int maxIterations, int minSet, float epsilon)
{
    const int N = f->N;
    int mRansacMinInliers = minInliers, mRansacMaxIts = maxIterations;
    float mRansacEpsilon = epsilon;
    int nMinInliers = N * mRansacEpsilon;
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N)
        nIterations = 1;
    else
        nIterations = ceil(log(1 - probability) / log(1 - pow(mRansacEpsilon, 3)));
    int lo = nIterations < mRansacMaxIts ? nIterations : mRansacMaxIts;
    f->max_its = lo > 1 ? lo : 1;
    f->min_inliers = mRansacMinInliers;
    f->epsilon = mRansacEpsilon;
}

/* The fold of the original iterate (:170-263) over hypotheses h = f->iterations ...: counts[h], nrefined[h] (of the hypotheses that
 * are records under this fold's own running best; a hypothesis that passes min_inliers without a record repeats the last Refine).
 * Returns the hypothesis whose result iterate returns, or -1; *kind = 1: its Refine succeeded (mRefinedTcw), 2: the best at the
 * end (mBestTcw), 0: an empty Mat.  available = number of hypotheses in counts (the fold never reads past it: the caller sizes it). */
int pno_iterate(pno_fold *f, const int32_t *counts, const int32_t *nrefined, int available, int nIterations, int *bNoMore, int *nInliers, int *kind)
{
    *bNoMore = 0; *nInliers = 0; *kind = 0;
    if (f->N < f->min_inliers) { *bNoMore = 1; return -1; }
    int nCurrentIterations = 0;
    while (f->iterations < f->max_its || nCurrentIterations < nIterations) {
        const int h = f->iterations;
        if (h >= available) return -2;
        nCurrentIterations++;
        f->iterations++;
        if (counts[h] >= f->min_inliers) {
            if (counts[h] > f->best_inliers) {
                f->best_inliers = counts[h];
                f->best = h;
                f->last_refined = nrefined[h];          /* Refine() on the new mvbBestInliers */
            }
            if (f->last_refined > f->min_inliers) {     /* Refine() on an unchanged mvbBestInliers repeats its result */
                *nInliers = f->last_refined; *kind = 1;
                return f->best;
            }
        }
    }
    if (f->iterations >= f->max_its) {
        *bNoMore = 1;
        if (f->best_inliers >= f->min_inliers) {
            *nInliers = f->best_inliers; *kind = 2;
            return f->best;
        }
    }
    return -1;
}

/* The fold of the first stage of iterate(Frame &, .., Map *) (:267-416): mnIterations restarts at 0; every hypothesis with
 * 2 < count < min_inliers is recorded (poses [npos] = its index, in order); a record whose Refine succeeds asks the caller's
 * projection search: accept[h] != 0 stands for nMatched >= 12.  Returns the accepted hypothesis or -1. */
int pno_iterate_frame_stage1(pno_fold *f, const int32_t *counts, const int32_t *nrefined, const uint8_t *accept, int available, int nIterations,
                             int32_t *poses, int *npos)
{
    f->iterations = 0;
    *npos = 0;
    int nCurrentIterations = 0;
    while (f->iterations < f->max_its || nCurrentIterations < nIterations) {
        const int h = f->iterations;
        if (h >= available) return -2;
        nCurrentIterations++;
        f->iterations++;
        if (counts[h] > 2 && counts[h] < f->min_inliers) poses[(*npos)++] = h;
        if (counts[h] >= f->min_inliers) {
            if (counts[h] > f->best_inliers) {
                f->best_inliers = counts[h];
                f->best = h;
                f->last_refined = nrefined[h];
            }
            if (f->last_refined > f->min_inliers && accept[f->best]) return f->best;
        }
    }
    return -1;
}
