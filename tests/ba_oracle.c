/* TEST INFRASTRUCTURE -- never part of the product.
 *
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:837-1162) and Optimizer::BundleAdjustment (:74-262) restated for the CPU on the
 * flattened graph of include/orbslam_hip.h (orbm_ba_graph), independent of the library: it includes none of its headers, its loops
 * run over run-time dimensions (2 rows for EdgeSE3ProjectXYZ, 3 for EdgeStereoSE3ProjectXYZ) and its sums run in g2o's orders:
 *   computeActiveErrors / activeRobustChi2   over the active edges in edge order, one running sum
 *   buildSystem                              edge after edge: Hll / bl of the point, Hpp / bp of the pose, the 6 x 3 Hpl block
 *   BlockSolver::solve (block_solver.hpp:354-496)   landmark after landmark: Dinv = (Hll + lambda I)^-1 (Eigen's fixed 3 x 3 inverse),
 *                                            Hschur block -= (B_i1 Dinv) B_i2^T, coefficients += B_i (Dinv bl), bschur = b - coefficients
 *   the reduced solve                        a dense LLT of the lower triangle, every entry's dot product from k = 0 upwards (this
 *                                            stands in for LinearSolverEigen's sparse LLT, as the library's does), then L y = b and
 *                                            L^T x = y column after column
 *   computeScale                             one running sum over the whole update vector, poses then points
 *   OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:63-241, bInFEA false) and SparseOptimizer::optimize's
 *   loop with its break at the first result that is not OK.
 * Poses are unit quaternions with g2o's normalisation after exp and every product (se3quat.h; Eigen's part: g2o_restated.h).
 *
 * The stop flag is modelled by a count: it reads as set from its stop_at-th read on (0: never); the reads are where g2o and
 * LocalBundleAdjustment make them.  Test-only switch: bao_set_ulp(seed != 0) moves every sin / cos / pow result of the exp map by
 * +1 or -1 ulp under a xorshift pattern of the seed. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "g2o_restated.h"

typedef struct {
    int32_t nfree, nfixed, npoints, nedges;
    const float *poses;
    const uint8_t *fixed;
    const float *points;
    const int32_t *e_point, *e_cam;
    const float *e_obs, *e_inv_sigma2, *e_cam_k;
} bao_graph;
typedef struct {
    int32_t nrounds, iterations[2], robust_round0, classify, reserved;
    double huber_mono, huber_stereo, chi2_mono, chi2_stereo;
} bao_options;
typedef struct { double tempChi, currentChi, rho, lambda, scale; int32_t round, qmax, accepted, ok2; } bao_trial;
typedef struct {
    float *poses, *points;              /* [nfree][16], [npoints][3] */
    uint8_t *erase, *not_included;      /* [nedges], [npoints] */
    int32_t stopped;
    int32_t rounds, iterations[2], trials[2], nresults, results[128];
    int32_t trial_capacity, ntrials, nreads;
    bao_trial *trial_log;
    double *poses_d, *points_d, *chi2;  /* [nfree][7], [npoints][3], [nedges] */
    uint8_t *level;                     /* [nedges] */
    double lambda_init[2];              /* computeLambdaInit of each round */
    double chi2_round1_start;           /* the plain chi2 over the level-0 edges at the start of round 1 (0 without one) */
} bao_out;

static uint64_t g_ulp;
void bao_set_ulp(uint64_t seed) { g_ulp = seed; }
static double ulp(double v)
{
    if (!g_ulp) return v;
    g_ulp ^= g_ulp << 13; g_ulp ^= g_ulp >> 7; g_ulp ^= g_ulp << 17;
    return nextafter(v, (g_ulp >> 11) & 1 ? INFINITY : -INFINITY);
}

typedef struct { double q[4], t[3]; } se3;

static void normalize_rotation(double q[4])
{
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] *= -1;
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n > 0.0) { const double s = sqrt(n); for (int i = 0; i < 4; ++i) q[i] /= s; }
}
static void quat_to_matrix(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
static void se3_map(const se3 *T, const double X[3], double o[3])
{
    q_rotate(T->q, X, o);
    for (int i = 0; i < 3; ++i) o[i] += T->t[i];
}
static void se3_exp(const double u[6], se3 *T)                  /* SE3Quat::exp */
{
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double Om[9] = {0., -u[2], u[1], u[2], 0., -u[0], -u[1], u[0], 0.};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k]; V[k] = R[k]; }
    } else {
        const double sn = ulp(sin(theta)), cs = ulp(cos(theta));
        const double a = sn / theta, b = (1 - cs) / (theta * theta), c = (theta - sn) / ulp(pow(theta, 3.0));
        for (int k = 0; k < 9; ++k) {
            const double I = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = I + a * Om[k] + b * O2[k];
            V[k] = I + b * Om[k] + c * O2[k];
        }
    }
    quat_from_matrix(R, T->q);
    for (int i = 0; i < 3; ++i) T->t[i] = V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
    normalize_rotation(T->q);
}
static void se3_compose(const se3 *A, const se3 *B, se3 *O)     /* SE3Quat::operator* */
{
    se3 r = *A;
    double rt[3];
    q_rotate(A->q, B->t, rt);
    for (int i = 0; i < 3; ++i) r.t[i] += rt[i];
    q_mul(A->q, B->q, r.q);
    normalize_rotation(r.q);
    *O = r;
}
static void se3_from_cv(const float *T, se3 *o)                 /* Converter::toSE3Quat */
{
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    quat_from_matrix(R, o->q);
    o->t[0] = T[3]; o->t[1] = T[7]; o->t[2] = T[11];
    normalize_rotation(o->q);
}

static void inverse3(const double *m, double *o)                /* Eigen compute_inverse<Matrix3d> */
{
#define M(i, j) m[3 * (i) + (j)]
#define COF(i, j) (M(((i) + 1) % 3, ((j) + 1) % 3) * M(((i) + 2) % 3, ((j) + 2) % 3) - M(((i) + 1) % 3, ((j) + 2) % 3) * M(((i) + 2) % 3, ((j) + 1) % 3))
    const double c0 = COF(0, 0), c1 = COF(1, 0), c2 = COF(2, 0);
    const double det = (c0 * M(0, 0) + c1 * M(1, 0)) + c2 * M(2, 0);
    const double invdet = 1.0 / det;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) o[3 * j + i] = (j == 0 ? (i == 0 ? c0 : i == 1 ? c1 : c2) : COF(i, j)) * invdet;
#undef COF
#undef M
}

static void huber(double e, double delta, double *rho0, double *rho1)      /* RobustKernelHuber::robustify */
{
    const float dsqr = (float)(delta * delta);
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
    else { const double sq = sqrt(e); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

/* one problem's state */
typedef struct {
    const bao_graph *g;
    const bao_options *o;
    int npose, nact, n;
    se3 *est, *est_bak;
    double *X, *X_bak, *err, *Hll, *bl, *Dinv, *db, *Hpl, *Hpp, *bp, *S, *bs, *x, *xl;
    uint8_t *level, *pact;
    int *ridx, *e_start;
    int stop_at, nreads, stop_seen;
} bao_state;

static int terminate(bao_state *s)
{
    ++s->nreads;
    if (s->stop_at && s->nreads >= s->stop_at) { s->stop_seen = 1; return 1; }
    return 0;
}
static int dims(const bao_graph *g, int e) { return g->e_obs[3 * e + 2] < 0.f ? 2 : 3; }

/* computeError: mono types_six_dof_expmap.h:95-100, stereo cam_project .cpp:150-157 with its float invz */
static void edge_error(const bao_state *s, int e, double c[3], double err[3])
{
    const bao_graph *g = s->g;
    const float *obs = g->e_obs + 3 * e, *K = g->e_cam_k + 5 * e;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    se3_map(&s->est[g->e_cam[e]], s->X + 3 * g->e_point[e], c);
    if (dims(g, e) == 2) {
        err[0] = (double)obs[0] - (c[0] / c[2] * fx + cx);
        err[1] = (double)obs[1] - (c[1] / c[2] * fy + cy);
        err[2] = 0.0;
    } else {
        const float invz = 1.0f / c[2];
        double res[3];
        res[0] = c[0] * invz * fx + cx;
        res[1] = c[1] * invz * fy + cy;
        res[2] = res[0] - K[4] * invz;
        for (int i = 0; i < 3; ++i) err[i] = (double)obs[i] - res[i];
    }
}
static double edge_chi2(const bao_state *s, int e)               /* chi2() of the STORED error */
{
    const double info = s->g->e_inv_sigma2[e], *err = s->err + 3 * e;
    double c = 0;
    for (int d = 0; d < dims(s->g, e); ++d) c = d ? c + err[d] * (info * err[d]) : err[d] * (info * err[d]);
    return c;
}
static double delta_of(const bao_state *s, int e) { return dims(s->g, e) == 2 ? s->o->huber_mono : s->o->huber_stereo; }

static double compute_active_errors(bao_state *s, int robust)   /* returns activeRobustChi2 */
{
    double chi = 0;
    for (int e = 0; e < s->g->nedges; ++e) {
        if (s->level[e]) continue;
        double c[3];
        edge_error(s, e, c, s->err + 3 * e);
        double c2 = edge_chi2(s, e), r0 = c2, r1;
        if (robust) huber(c2, delta_of(s, e), &r0, &r1);
        chi += r0;
    }
    return chi;
}

static void jacobians(const bao_state *s, int e, double A[9], double B[18])
{
    const bao_graph *g = s->g;
    const float *K = g->e_cam_k + 5 * e;
    const double fx = K[0], fy = K[1], bf = K[4];
    const se3 *T = &s->est[g->e_cam[e]];
    double c[3], R[9];
    se3_map(T, s->X + 3 * g->e_point[e], c);
    quat_to_matrix(T->q, R);
    const double x = c[0], y = c[1], z = c[2], z_2 = z * z;
    memset(A, 0, sizeof(double) * 9); memset(B, 0, sizeof(double) * 18);
    if (dims(g, e) == 2) {                                      /* .cpp:103-139 */
        const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 3; ++j) A[3 * i + j] = -1. / z * (tmp[3 * i] * R[j] + tmp[3 * i + 1] * R[3 + j] + tmp[3 * i + 2] * R[6 + j]);
    } else {                                                    /* .cpp:188-234 */
        for (int j = 0; j < 3; ++j) {
            A[j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
            A[3 + j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
            A[6 + j] = A[j] - bf * R[6 + j] / z_2;
        }
    }
    B[0] = x * y / z_2 * fx; B[1] = -(1 + (x * x / z_2)) * fx; B[2] = y / z * fx; B[3] = -1. / z * fx; B[4] = 0; B[5] = x / z_2 * fx;
    B[6] = (1 + y * y / z_2) * fy; B[7] = -x * y / z_2 * fy; B[8] = -x / z * fy; B[9] = 0; B[10] = -1. / z * fy; B[11] = y / z_2 * fy;
    if (dims(g, e) == 3) {
        B[12] = B[0] - bf * y / z_2; B[13] = B[1] + bf * x / z_2; B[14] = B[2]; B[15] = B[3]; B[16] = 0; B[17] = B[5] - bf / z_2;
    }
}

/* initializeOptimization(level 0): the vertices with a level-0 edge; returns the number of active edges */
static int activate(bao_state *s)
{
    const bao_graph *g = s->g;
    int nedges = 0;
    memset(s->pact, 0, (size_t)g->npoints);
    for (int p = 0; p < g->nfree; ++p) s->ridx[p] = -1;
    for (int e = 0; e < g->nedges; ++e) {
        if (s->level[e]) continue;
        ++nedges;
        s->pact[g->e_point[e]] = 1;
        const int c = g->e_cam[e];
        if (c < g->nfree && !(g->fixed && g->fixed[c])) s->ridx[c] = 0;
    }
    s->nact = 0;
    for (int p = 0; p < g->nfree; ++p)
        if (s->ridx[p] == 0) s->ridx[p] = s->nact++;
    s->n = 6 * s->nact;
    return nedges;
}
static int free_row(const bao_state *s, int e)
{
    const int c = s->g->e_cam[e];
    return c < s->g->nfree ? s->ridx[c] : -1;
}

static double build_system(bao_state *s, int robust)            /* returns computeLambdaInit's largest diagonal entry */
{
    const bao_graph *g = s->g;
    memset(s->Hll, 0, sizeof(double) * 9 * g->npoints); memset(s->bl, 0, sizeof(double) * 3 * g->npoints);
    memset(s->Hpp, 0, sizeof(double) * 36 * (s->nact ? s->nact : 1)); memset(s->bp, 0, sizeof(double) * 6 * (s->nact ? s->nact : 1));
    for (int e = 0; e < g->nedges; ++e) {
        if (s->level[e]) continue;
        const int D = dims(g, e), pt = g->e_point[e], r = free_row(s, e);
        const double info = g->e_inv_sigma2[e], *err = s->err + 3 * e;
        double A[9], B[18], rho0, rho1 = 1.;
        jacobians(s, e, A, B);
        if (robust) huber(edge_chi2(s, e), delta_of(s, e), &rho0, &rho1);
        const double w = rho1 * info;
        double wr[3];
        for (int d = 0; d < D; ++d) wr[d] = -(info * err[d]) * rho1;
        for (int i = 0; i < 3; ++i) {
            double a = A[i] * wr[0];
            for (int d = 1; d < D; ++d) a += A[3 * d + i] * wr[d];
            s->bl[3 * pt + i] += a;
            for (int j = 0; j < 3; ++j) {
                double h = A[i] * w * A[j];
                for (int d = 1; d < D; ++d) h += A[3 * d + i] * w * A[3 * d + j];
                s->Hll[9 * pt + 3 * i + j] += h;
            }
        }
        if (r < 0) continue;
        double *hp = s->Hpl + 18 * e;
        for (int i = 0; i < 6; ++i) {
            double a = B[i] * wr[0];
            for (int d = 1; d < D; ++d) a += B[6 * d + i] * wr[d];
            s->bp[6 * r + i] += a;
            for (int j = 0; j <= i; ++j) {
                double h = B[i] * w * B[j];
                for (int d = 1; d < D; ++d) h += B[6 * d + i] * w * B[6 * d + j];
                s->Hpp[36 * r + 6 * i + j] += h;
            }
            for (int q = 0; q < 3; ++q) {
                double h = B[i] * w * A[q];
                for (int d = 1; d < D; ++d) h += B[6 * d + i] * w * A[3 * d + q];
                hp[3 * i + q] = h;
            }
        }
    }
    double maxd = 0;
    for (int r = 0; r < s->nact; ++r)
        for (int i = 0; i < 6; ++i) maxd = fmax(fabs(s->Hpp[36 * r + 7 * i]), maxd);
    for (int n = 0; n < g->npoints; ++n)
        if (s->pact[n])
            for (int i = 0; i < 3; ++i) maxd = fmax(fabs(s->Hll[9 * n + 4 * i]), maxd);
    return maxd;
}

/* BlockSolver::solve with the dense LLT; x = poses' update, xl = points'; returns ok2 */
static int solve(bao_state *s, double lambda)
{
    const bao_graph *g = s->g;
    const int n = s->n;
    double *S = s->S;                                           /* row-major, the lower triangle is used */
    for (int i = 0; i < n * n; ++i) S[i] = 0.0;
    for (int r = 0; r < s->nact; ++r)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j <= i; ++j) S[(6 * r + i) * n + 6 * r + j] = s->Hpp[36 * r + 6 * i + j] + (i == j ? lambda : 0.0);
    double *coef = s->bs;
    for (int i = 0; i < n; ++i) coef[i] = 0.0;
    for (int pt = 0; pt < g->npoints; ++pt) {
        if (!s->pact[pt]) continue;
        double M[9], *inv = s->Dinv + 9 * pt, *db = s->db + 3 * pt;
        for (int j = 0; j < 9; ++j) M[j] = s->Hll[9 * pt + j];
        for (int j = 0; j < 3; ++j) M[4 * j] += lambda;
        inverse3(M, inv);
        for (int j = 0; j < 3; ++j) db[j] = inv[3 * j] * s->bl[3 * pt] + inv[3 * j + 1] * s->bl[3 * pt + 1] + inv[3 * j + 2] * s->bl[3 * pt + 2];
        for (int a = s->e_start[pt]; a < s->e_start[pt + 1]; ++a) {
            const int ra = s->level[a] ? -1 : free_row(s, a);
            if (ra < 0) continue;
            const double *h1 = s->Hpl + 18 * a;
            double W[18];                                       /* BDinv = Bi * Dinv */
            for (int i = 0; i < 6; ++i)
                for (int k = 0; k < 3; ++k) W[3 * i + k] = h1[3 * i] * inv[k] + h1[3 * i + 1] * inv[3 + k] + h1[3 * i + 2] * inv[6 + k];
            for (int i = 0; i < 6; ++i) coef[6 * ra + i] += h1[3 * i] * db[0] + h1[3 * i + 1] * db[1] + h1[3 * i + 2] * db[2];
            for (int b = s->e_start[pt]; b < s->e_start[pt + 1]; ++b) {
                const int rb = s->level[b] ? -1 : free_row(s, b);
                if (rb < ra) continue;                          /* (also rb = -1) the upper blocks i1 <= i2; stored transposed */
                const double *h2 = s->Hpl + 18 * b;
                for (int i = 0; i < 6; ++i)
                    for (int c = 0; c < 6; ++c) {
                        const int row = 6 * rb + c, col = 6 * ra + i;
                        if (row < col) continue;
                        S[row * n + col] -= W[3 * i] * h2[3 * c] + W[3 * i + 1] * h2[3 * c + 1] + W[3 * i + 2] * h2[3 * c + 2];
                    }
            }
        }
    }
    for (int r = 0; r < s->nact; ++r)
        for (int i = 0; i < 6; ++i) s->bs[6 * r + i] = s->bp[6 * r + i] - coef[6 * r + i];
    /* LLT, lower triangle, column after column */
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) {
            double v = S[i * n + j];
            if (j > 0) {
                double dot = S[i * n] * S[j * n];
                for (int k = 1; k < j; ++k) dot = dot + S[i * n + k] * S[j * n + k];
                v = v - dot;
            }
            if (i == j) {
                if (!(v > 0.0)) return 0;
                S[j * n + j] = sqrt(v);
            } else
                S[i * n + j] = v / S[j * n + j];
        }
    double *y = s->x;
    for (int i = 0; i < n; ++i) y[i] = s->bs[i];
    for (int j = 0; j < n; ++j) {
        y[j] = y[j] / S[j * n + j];
        for (int i = j + 1; i < n; ++i) y[i] -= S[i * n + j] * y[j];
    }
    for (int j = n - 1; j >= 0; --j) {
        y[j] = y[j] / S[j * n + j];
        for (int i = 0; i < j; ++i) y[i] -= S[j * n + i] * y[j];
    }
    /* cl = bl - B^T xp, xl = Dinv cl */
    for (int pt = 0; pt < g->npoints; ++pt) {
        double *xl = s->xl + 3 * pt;
        xl[0] = xl[1] = xl[2] = 0.0;
        if (!s->pact[pt]) continue;
        double cl[3] = {s->bl[3 * pt], s->bl[3 * pt + 1], s->bl[3 * pt + 2]};
        for (int a = s->e_start[pt]; a < s->e_start[pt + 1]; ++a) {
            const int ra = s->level[a] ? -1 : free_row(s, a);
            if (ra < 0) continue;
            const double *hp = s->Hpl + 18 * a;
            for (int q = 0; q < 6; ++q) {
                const double cp = -s->x[6 * ra + q];
                for (int j = 0; j < 3; ++j) cl[j] = cl[j] + hp[3 * q + j] * cp;
            }
        }
        const double *inv = s->Dinv + 9 * pt;
        for (int j = 0; j < 3; ++j) xl[j] = inv[3 * j] * cl[0] + inv[3 * j + 1] * cl[1] + inv[3 * j + 2] * cl[2];
    }
    return 1;
}

/* SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve */
static void optimize(bao_state *s, int round, bao_out *out)
{
    const bao_graph *g = s->g;
    const int robust = round == 0 && s->o->robust_round0;
    double lambda = -1., ni = 2.;
    int nbad = 0, ok = 1;
    for (int it = 0; it < s->o->iterations[round] && !terminate(s) && ok; ++it) {
        double currentChi = compute_active_errors(s, robust);
        double tempChi = currentChi;
        const double iniChi = currentChi;
        const double maxd = build_system(s, robust);
        if (it == 0) { lambda = 1e-5 * maxd; ni = 2; nbad = 0; out->lambda_init[round] = lambda; }
        double rho = 0;
        int qmax = 0;
        do {
            for (int p = 0; p < g->nfree; ++p) s->est_bak[p] = s->est[p];                      /* push */
            memcpy(s->X_bak, s->X, sizeof(double) * 3 * g->npoints);
            const int ok2 = solve(s, lambda);
            double scale = 0.;
            if (ok2) {                                                                          /* update(x) */
                for (int p = 0; p < g->nfree; ++p) {
                    if (s->ridx[p] < 0) continue;
                    se3 up;
                    se3_exp(s->x + 6 * s->ridx[p], &up);
                    se3_compose(&up, &s->est_bak[p], &s->est[p]);
                }
                for (int pt = 0; pt < g->npoints; ++pt)
                    if (s->pact[pt])
                        for (int j = 0; j < 3; ++j) s->X[3 * pt + j] += s->xl[3 * pt + j];
                for (int j = 0; j < s->n; ++j) scale += s->x[j] * (lambda * s->x[j] + s->bp[j]);   /* computeScale */
                for (int pt = 0; pt < g->npoints; ++pt)
                    if (s->pact[pt])
                        for (int j = 0; j < 3; ++j) scale += s->xl[3 * pt + j] * (lambda * s->xl[3 * pt + j] + s->bl[3 * pt + j]);
            }
            tempChi = compute_active_errors(s, robust);
            if (!ok2) tempChi = DBL_MAX;
            rho = (currentChi - tempChi);
            scale += 1e-3;
            rho /= scale;
            const int good = rho > 0 && isfinite(tempChi);
            if (good) {
                double alpha = 1. - pow((2 * rho - 1), 3);
                alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
                const double scaleFactor = 1. / 3. < alpha ? alpha : 1. / 3.;
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                for (int p = 0; p < g->nfree; ++p) s->est[p] = s->est_bak[p];                  /* pop */
                memcpy(s->X, s->X_bak, sizeof(double) * 3 * g->npoints);
            }
            if (out->ntrials < out->trial_capacity) {
                bao_trial *t = &out->trial_log[out->ntrials];
                t->tempChi = tempChi; t->currentChi = currentChi; t->rho = rho; t->lambda = lambda; t->scale = scale;
                t->round = round; t->qmax = qmax; t->accepted = good; t->ok2 = ok2;
            }
            out->ntrials++;
            qmax++;
        } while (rho < 0 && qmax < 10 && !terminate(s));
        out->iterations[round]++;
        out->trials[round] += qmax;
        int result;
        if (qmax == 10 || rho == 0) result = 2;
        else {
            if ((iniChi - currentChi) * 1e3 < iniChi) nbad++;
            else nbad = 0;
            result = nbad >= 3 ? 2 : 1;
        }
        if (out->nresults < 128) out->results[out->nresults] = result;
        out->nresults++;
        ok = result == 1;
    }
}

static int is_bad(const bao_state *s, int e)                     /* chi2() > th || !isDepthPositive() */
{
    double c[3];
    se3_map(&s->est[s->g->e_cam[e]], s->X + 3 * s->g->e_point[e], c);
    const double th = dims(s->g, e) == 2 ? s->o->chi2_mono : s->o->chi2_stereo;
    return edge_chi2(s, e) > th || !(c[2] > 0.0);
}

int bao_run(const bao_graph *g, const bao_options *o, int stop_at, bao_out *out)
{
    bao_state s;
    memset(&s, 0, sizeof(s));
    s.g = g; s.o = o; s.npose = g->nfree + g->nfixed; s.stop_at = stop_at;
    const int np = g->npoints, ne = g->nedges, nf = g->nfree, nmax = 6 * nf;
    out->stopped = 0; out->rounds = 0; out->nresults = 0; out->ntrials = 0; out->nreads = 0;
    out->lambda_init[0] = out->lambda_init[1] = 0; out->chi2_round1_start = 0;
    for (int r = 0; r < 2; ++r) { out->iterations[r] = 0; out->trials[r] = 0; }
    memset(out->results, 0, sizeof(out->results));
    memcpy(out->poses, g->poses, sizeof(float) * 16 * nf);
    memcpy(out->points, g->points, sizeof(float) * 3 * np);
    if (out->erase) memset(out->erase, 0, (size_t)ne);
    s.e_start = calloc((size_t)np + 1, sizeof(int));
    for (int e = 0; e < ne; ++e) s.e_start[g->e_point[e] + 1]++;
    for (int n = 0; n < np; ++n) {
        if (out->not_included) out->not_included[n] = s.e_start[n + 1] == 0;
        s.e_start[n + 1] += s.e_start[n];
    }
#define ALLOC(T, n) ((T *)calloc((size_t)(n) + 1, sizeof(T)))
    s.est = ALLOC(se3, s.npose); s.est_bak = ALLOC(se3, nf); s.X = ALLOC(double, 3 * np); s.X_bak = ALLOC(double, 3 * np);
    s.err = ALLOC(double, 3 * ne); s.Hll = ALLOC(double, 9 * np); s.bl = ALLOC(double, 3 * np); s.Dinv = ALLOC(double, 9 * np);
    s.db = ALLOC(double, 3 * np); s.Hpl = ALLOC(double, 18 * ne); s.Hpp = ALLOC(double, 36 * nf); s.bp = ALLOC(double, nmax);
    s.S = ALLOC(double, (size_t)nmax * nmax); s.bs = ALLOC(double, nmax); s.x = ALLOC(double, nmax); s.xl = ALLOC(double, 3 * np);
    s.level = ALLOC(uint8_t, ne); s.pact = ALLOC(uint8_t, np); s.ridx = ALLOC(int, nf);
    for (int p = 0; p < s.npose; ++p) se3_from_cv(g->poses + 16 * p, &s.est[p]);
    for (int i = 0; i < 3 * np; ++i) s.X[i] = g->points[i];
    int nedges = activate(&s);
    int ran = 0;
    if (nf == 0 || ne == 0 || s.nact == 0) goto done;           /* nothing to optimise: the input comes back */
    if (terminate(&s)) { out->stopped = 1; goto done; }         /* Optimizer.cc:1039-1041 */
    ran = 1;
    for (int round = 0; round < o->nrounds; ++round) {
        if (s.nact > 0 && nedges > 0) {
            if (round == 1) {
                double c[3], e3[3], chi = 0;
                for (int e = 0; e < ne; ++e) {
                    if (s.level[e]) continue;
                    const double info = g->e_inv_sigma2[e];
                    edge_error(&s, e, c, e3);
                    for (int d = 0; d < dims(g, e); ++d) chi += e3[d] * (info * e3[d]);
                }
                out->chi2_round1_start = chi;
            }
            out->rounds++;
            optimize(&s, round, out);
        }
        if (round + 1 < o->nrounds) {
            if (terminate(&s)) break;                           /* :1046-1049: bDoMore = false, read behind optimize(5); no level pass */
            if (o->classify)
                for (int e = 0; e < ne; ++e)
                    if (is_bad(&s, e)) s.level[e] = 1;
            nedges = activate(&s);
        }
    }
    if (o->classify)
        for (int e = 0; e < ne; ++e) out->erase[e] = (uint8_t)is_bad(&s, e);
    for (int p = 0; p < nf; ++p) {                              /* Converter::toCvMat, every local keyframe (:1146-1152) */
        double R[9];
        quat_to_matrix(s.est[p].q, R);
        float *T = out->poses + 16 * p;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)s.est[p].t[r];
        }
        T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
    }
    for (int n = 0; n < np; ++n)
        if (s.e_start[n + 1] > s.e_start[n])
            for (int j = 0; j < 3; ++j) out->points[3 * n + j] = (float)s.X[3 * n + j];
    if (s.stop_seen) out->stopped = 2;
done:
    (void)ran;
    out->nreads = s.nreads;
    for (int p = 0; out->poses_d && p < nf; ++p) {
        for (int j = 0; j < 4; ++j) out->poses_d[7 * p + j] = ran ? s.est[p].q[j] : 0.0;
        for (int j = 0; j < 3; ++j) out->poses_d[7 * p + 4 + j] = ran ? s.est[p].t[j] : 0.0;
    }
    for (int i = 0; out->points_d && i < 3 * np; ++i) out->points_d[i] = s.X[i];
    for (int e = 0; e < ne; ++e) {
        if (out->chi2) out->chi2[e] = ran ? edge_chi2(&s, e) : 0.0;
        if (out->level) out->level[e] = s.level[e];
    }
    free(s.e_start); free(s.est); free(s.est_bak); free(s.X); free(s.X_bak); free(s.err); free(s.Hll); free(s.bl); free(s.Dinv); free(s.db);
    free(s.Hpl); free(s.Hpp); free(s.bp); free(s.S); free(s.bs); free(s.x); free(s.xl); free(s.level); free(s.pact); free(s.ridx);
    return 0;
}
