/* sim3_opt_oracle.c -- CPU restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1425-1625) from :1564 on: the two optimisation
 * rounds, the outlier cut between them and the final count, on g2o's code paths (test infrastructure, never part of the product):
 *   Thirdparty/g2o/g2o/types/sim3.h:59-67 (Sim3 from R, t, s), :70-142 (Sim3(Vector7d)), :144-146 (map), :233-236 (inverse),
 *     :266-272 (operator*)
 *   types/types_seven_dof_expmap.h:60-69 (oplusImpl with _fix_scale), :138-145 / :160-167 (computeError of both edges)
 *   types/se3_ops.hpp:27-38 (skew), :49-55 (project)
 *   core/base_binary_edge.hpp:55-120 (constructQuadraticForm, robust branch), :131-205 (the numeric linearizeOplus)
 *   core/robust_kernel_impl.cpp (Huber), core/optimization_algorithm_levenberg.cpp:63-268, core/sparse_optimizer.cpp:425-504
 *   solvers/linear_solver_dense.h:64-112 with Eigen 3.3's LDLT (ldlt_inplace, diagonal pivoting, lower triangle) and isPositive()
 * Sums run in g2o's order: the active edges in creation order, e12 then e21 of a pair.  Eigen's quaternion constructor, products
 * and rotation are restated as orbm_pose.hip restates them.
 *
 * Test-only switch: s3x_set_ulp(seed != 0) moves every sin / cos / exp result by +1 or -1 ulp under a xorshift pattern of the
 * seed; tests/test_cpu_sim3_opt.py measures with it how far the result moves when the last bit of those functions does. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "g2o_restated.h"              /* Eigen: Quaterniond(Matrix3d), quaternion product, quaternion * vector, LDLT */

typedef struct { double q[4], t[3], s; } s3x_sim3;   /* q = x y z w */

typedef struct {                                      /* = orbm_sim3_opt_result */
    double q[4], t[3], s;
    int32_t nin, nbad, ncorrespondences;
    int32_t iterations[2], trials[2];
    double chi2;
} s3x_result;

static uint64_t g_ulp;                                /* 0: off */
void s3x_set_ulp(uint64_t seed) { g_ulp = seed; }
static double jig(double v)
{
    if (!g_ulp) return v;
    g_ulp ^= g_ulp << 13; g_ulp ^= g_ulp >> 7; g_ulp ^= g_ulp << 17;
    return nextafter(v, (g_ulp >> 11) & 1 ? INFINITY : -INFINITY);
}
static double p_sin(double x) { return jig(sin(x)); }
static double p_cos(double x) { return jig(cos(x)); }
static double p_exp(double x) { return jig(exp(x)); }

/* ---- sim3.h */
void s3x_from_rts(const float R[9], const float t[3], float s, s3x_sim3 *o)      /* :64-67 behind Converter::toMatrix3d / toVector3d */
{
    double Rd[9];
    for (int k = 0; k < 9; ++k) Rd[k] = R[k];
    quat_from_matrix(Rd, o->q);
    for (int k = 0; k < 3; ++k) o->t[k] = t[k];
    o->s = s;
}

void s3x_exp(const double u[7], s3x_sim3 *o)                                      /* :70-142 */
{
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double Om[9] = {0., -w2, w1, w2, 0., -w0, -w1, w0, 0.};
    const double s = p_exp(sigma);
    double O2[9], R[9], A, B, C;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    const double eps = 0.00001;
    const int small_theta = theta < eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - p_cos(theta)) / (theta2);
            B = (theta - p_sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * p_sin(theta), b = s * p_cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    if (small_theta) {                                   /* the first-order rotation, not orthogonal; its quaternion is not normalised */
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
    } else {
        const double ra = p_sin(theta) / theta, rb = (1 - p_cos(theta)) / (theta * theta);
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + ra * Om[k] + rb * O2[k];
    }
    quat_from_matrix(R, o->q);
    double W[9];
    for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + B * O2[k] + C * ((k % 4 == 0) ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) o->t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o->s = s;
}

void s3x_mul(const s3x_sim3 *a, const s3x_sim3 *b, s3x_sim3 *o)                   /* :266-272 */
{
    s3x_sim3 r;
    double rt[3];
    q_mul(a->q, b->q, r.q);
    q_rotate(a->q, b->t, rt);
    for (int k = 0; k < 3; ++k) r.t[k] = a->s * rt[k] + a->t[k];
    r.s = a->s * b->s;
    *o = r;
}

void s3x_inverse(const s3x_sim3 *a, s3x_sim3 *o)                                  /* :233-236 */
{
    s3x_sim3 r;
    const double f = -1. / a->s;
    const double v[3] = {f * a->t[0], f * a->t[1], f * a->t[2]};
    r.q[0] = -a->q[0]; r.q[1] = -a->q[1]; r.q[2] = -a->q[2]; r.q[3] = a->q[3];
    q_rotate(r.q, v, r.t);
    r.s = 1. / a->s;
    *o = r;
}

void s3x_map(const s3x_sim3 *a, const double X[3], double o[3])                   /* :144-146 */
{
    double r[3];
    q_rotate(a->q, X, r);
    for (int k = 0; k < 3; ++k) o[k] = a->s * r[k] + a->t[k];
}

/* LinearSolverDense's LDLT of a 7 x 7 matrix, in place, Eigen's way where the diagonal has no entry to pivot on (x is left as it is
 * when not isPositive()) */
static int ldlt_solve7(double m[49], const double b[7], double x[7]) { return ldlt_solve(m, b, 7, LDLT_AS_EIGEN, x); }
int s3x_ldlt7(const double *H, const double *b, double *x) { double m[49]; memcpy(m, H, sizeof(m)); return ldlt_solve7(m, b, x); }

/* ---- the edges */
typedef struct {
    int n, fix_scale;
    const double *P1, *P2;          /* [n][3] camera-frame points (vPoint1 / vPoint2) */
    const float *obs1, *obs2;       /* [n][2] */
    const float *info1, *info2;     /* [n] mvInvLevelSigma2[octave] */
    double f1[2], c1[2], f2[2], c2[2];
    double delta;                   /* RobustKernelHuber::_delta = (float)sqrt(th2) */
} prob_t;

/* computeError of EdgeSim3ProjectXYZ (inv = 0: S = the estimate) and EdgeInverseSim3ProjectXYZ (inv = 1: S = its inverse) */
static void edge_error(const s3x_sim3 *S, const double X[3], const float obs[2], const double f[2], const double c[2], double e[2])
{
    double p[3];
    s3x_map(S, X, p);
    const double u = p[0] / p[2], v = p[1] / p[2];
    e[0] = (double)obs[0] - (u * f[0] + c[0]);
    e[1] = (double)obs[1] - (v * f[1] + c[1]);
}

static double edge_chi2(double info, const double e[2])      /* _error.dot(information() * _error), information = info * I */
{
    const double o0 = info * e[0] + 0.0 * e[1], o1 = 0.0 * e[0] + info * e[1];
    return e[0] * o0 + e[1] * o1;
}

static void huber(double e, double delta, double *rho0, double *rho1)
{
    const float dsqr = (float)(delta * delta);
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
    else {
        const double sqrte = sqrt(e);
        *rho0 = 2 * sqrte * delta - dsqr;
        *rho1 = delta / sqrte;
    }
}

static void pair_errors(const prob_t *p, int i, const s3x_sim3 *S, const s3x_sim3 *Sinv, double e12[2], double e21[2])
{
    edge_error(S, p->P2 + 3 * i, p->obs1 + 2 * i, p->f1, p->c1, e12);
    edge_error(Sinv, p->P1 + 3 * i, p->obs2 + 2 * i, p->f2, p->c2, e21);
}

/* the 14 estimates of the numeric Jacobian (base_binary_edge.hpp:157-173 through oplusImpl): pe[2 d] = Sim3(+delta e_d) * est,
 * pe[2 d + 1] = Sim3(-delta e_d) * est, with update[6] = 0 under _fix_scale; pi = their inverses */
static void perturbed(const s3x_sim3 *est, int fix_scale, s3x_sim3 pe[14], s3x_sim3 pi[14])
{
    const double delta = 1e-9;
    for (int k = 0; k < 14; ++k) {
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[k >> 1] = (k & 1) ? -delta : delta;
        if (fix_scale) u[6] = 0;
        s3x_sim3 up;
        s3x_exp(u, &up);
        s3x_mul(&up, est, &pe[k]);
        s3x_inverse(&pe[k], &pi[k]);
    }
}

/* one edge into the system: J (numeric), robust chi2, H += J^T (rho1 info) J, b += J^T (rho1 * -(info e)) */
static void edge_system(const s3x_sim3 S[14], const s3x_sim3 *S0, const double X[3], const float obs[2], const double f[2], const double c[2],
                        double info, double delta_h, double H[49], double b[7], double *chi, double Jout[14])
{
    const double scalar = 1.0 / (2 * 1e-9);
    double e[2], J[2][7];
    edge_error(S0, X, obs, f, c, e);
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        edge_error(&S[2 * d], X, obs, f, c, ep);
        edge_error(&S[2 * d + 1], X, obs, f, c, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    double rho0, w;
    huber(edge_chi2(info, e), delta_h, &rho0, &w);
    *chi += rho0;
    const double winfo = w * info;
    const double r0 = -(info * e[0]) * w, r1 = -(info * e[1]) * w;
    for (int r = 0; r < 7; ++r) {
        b[r] += J[0][r] * r0 + J[1][r] * r1;
        for (int cc = 0; cc <= r; ++cc) H[7 * r + cc] += J[0][r] * (winfo * J[0][cc]) + J[1][r] * (winfo * J[1][cc]);
    }
    if (Jout) for (int d = 0; d < 7; ++d) { Jout[d] = J[0][d]; Jout[7 + d] = J[1][d]; }
}

/* linearizeOplus of one pair at `est` (test access): J12 [2][7], J21 [2][7] */
void s3x_linearize(const s3x_sim3 *est, int fix_scale, const double P1[3], const double P2[3], const float obs1[2], const float obs2[2],
                   const float cam1[4], const float cam2[4], double J12[14], double J21[14])
{
    s3x_sim3 pe[14], pi[14], inv;
    double H[49] = {0}, b[7] = {0}, chi = 0;
    const double f1[2] = {cam1[0], cam1[1]}, c1[2] = {cam1[2], cam1[3]}, f2[2] = {cam2[0], cam2[1]}, c2[2] = {cam2[2], cam2[3]};
    perturbed(est, fix_scale, pe, pi);
    s3x_inverse(est, &inv);
    edge_system(pe, est, P2, obs1, f1, c1, 1.0, 1.0, H, b, &chi, J12);
    edge_system(pi, &inv, P1, obs2, f2, c2, 1.0, 1.0, H, b, &chi, J21);
}

static double active_chi2(const prob_t *p, const uint8_t *active, const s3x_sim3 *S)
{
    s3x_sim3 inv;
    s3x_inverse(S, &inv);
    double chi = 0;
    for (int i = 0; i < p->n; ++i) {
        if (!active[i]) continue;
        double e12[2], e21[2], rho0, w;
        pair_errors(p, i, S, &inv, e12, e21);
        huber(edge_chi2(p->info1[i], e12), p->delta, &rho0, &w); chi += rho0;
        huber(edge_chi2(p->info2[i], e21), p->delta, &rho0, &w); chi += rho0;
    }
    return chi;
}

typedef struct {            /* what the tests look at besides the result */
    int32_t small_rho;      /* Levenberg trials with |rho| < 1e-9 */
    int32_t eval_is_est[2]; /* per round: the last tried estimate is the accepted one, bit for bit */
    double H6max, b6;       /* the largest |H(6, .)| and |b[6]| any buildSystem saw */
    double lambda0[2];      /* computeLambdaInit of each round */
    double min_abs_rho;     /* the smallest |rho| of any trial (NaN ones apart); +inf without a trial */
    int32_t hit_limit[2];   /* per round: optimize() ran out of iterations (no Terminate, no stop by Raul's criterion) */
} s3x_trace;

/* SparseOptimizer::optimize(maxit) over the active pairs; *eval: the estimate of the last computeActiveErrors */
static void run_round(const prob_t *p, const uint8_t *active, s3x_sim3 *est, s3x_sim3 *eval, int maxit, int32_t *iters_out, int32_t *trials_out,
                      double *chi_out, s3x_trace *tr, int round)
{
    double lambda = 0.0;
    int ni = 2, lmBad = 0, iters = 0, trials = 0, stopped = 0;
    for (int iteration = 0; iteration < maxit; ++iteration) {
        ++iters;
        s3x_sim3 pe[14], pi[14], inv;
        double H[49], bb[7], chi = 0;
        memset(H, 0, sizeof(H)); memset(bb, 0, sizeof(bb));
        perturbed(est, p->fix_scale, pe, pi);
        s3x_inverse(est, &inv);
        for (int i = 0; i < p->n; ++i) {
            if (!active[i]) continue;
            edge_system(pe, est, p->P2 + 3 * i, p->obs1 + 2 * i, p->f1, p->c1, p->info1[i], p->delta, H, bb, &chi, 0);
            edge_system(pi, &inv, p->P1 + 3 * i, p->obs2 + 2 * i, p->f2, p->c2, p->info2[i], p->delta, H, bb, &chi, 0);
        }
        *eval = *est;
        double currentChi = chi;
        const double iniChi = currentChi;
        if (tr) {
            for (int c = 0; c < 7; ++c) { const double f = fabs(H[42 + c]); if (f > tr->H6max) tr->H6max = f; }
            if (fabs(bb[6]) > tr->b6) tr->b6 = fabs(bb[6]);
        }
        if (iteration == 0) {                                   /* computeLambdaInit, tau = 1e-5 */
            double maxDiagonal = 0.;
            for (int j = 0; j < 7; ++j) { const double f = fabs(H[8 * j]); maxDiagonal = (f < maxDiagonal) ? maxDiagonal : f; }
            lambda = 1e-5 * maxDiagonal;
            ni = 2;
            lmBad = 0;
            if (tr) tr->lambda0[round] = lambda;
        }
        double rho = 0;
        int qmax = 0;
        do {
            double Hl[49], x[7] = {0, 0, 0, 0, 0, 0, 0};
            memcpy(Hl, H, sizeof(Hl));
            for (int j = 0; j < 7; ++j) Hl[8 * j] += lambda;
            const int ok2 = ldlt_solve7(Hl, bb, x);
            if (p->fix_scale) x[6] = 0;                         /* oplusImpl writes into the solver's x */
            s3x_sim3 up, trial;
            s3x_exp(x, &up);
            s3x_mul(&up, est, &trial);
            double tempChi = active_chi2(p, active, &trial);
            *eval = trial;
            if (!ok2) tempChi = 1.7976931348623157e308;
            rho = (currentChi - tempChi);
            double scale = 0.;
            for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + bb[j]);
            scale += 1e-3;
            rho /= scale;
            if (tr && fabs(rho) < 1e-9) tr->small_rho++;
            if (tr && fabs(rho) < tr->min_abs_rho) tr->min_abs_rho = fabs(rho);
            if (rho > 0 && isfinite(tempChi)) {
                double alpha = 1. - pow((2 * rho - 1), 3.0);
                alpha = (alpha < 2. / 3.) ? alpha : 2. / 3.;
                const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
                *est = trial;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        trials += qmax;
        *chi_out = currentChi;
        if (qmax == 10 || rho == 0) { stopped = 1; break; }     /* Terminate */
        if ((iniChi - currentChi) * 1e3 < iniChi) lmBad++;      /* Raul's stop criterion */
        else lmBad = 0;
        if (lmBad >= 3) { stopped = 1; break; }
    }
    *iters_out = iters; *trials_out = trials;
    if (tr) tr->hit_limit[round] = !stopped;
    if (tr) tr->eval_is_est[round] = memcmp(est, eval, sizeof(*est)) == 0;
}

/* vPoint1 / vPoint2 (Optimizer.cc:1501-1511): R * Xw + t as one cv::Mat gemm in float, widened */
void s3x_prepare(const float *Xw, const float *Tcw, int n, double *Xc)
{
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            const float row = Tcw[4 * r] * Xw[3 * i] + Tcw[4 * r + 1] * Xw[3 * i + 1] + Tcw[4 * r + 2] * Xw[3 * i + 2];
            Xc[3 * i + r] = (double)(float)((double)row * 1.0 + (double)Tcw[4 * r + 3] * 1.0);
        }
}

/* chi2 of both edges of every pair at S (test access): out [n][2] */
void s3x_pair_chi2(const double *P1, const double *P2, const float *obs1, const float *obs2, const float *info1, const float *info2, int n,
                   const float cam1[4], const float cam2[4], const s3x_sim3 *S, double *out)
{
    prob_t p = {n, 0, P1, P2, obs1, obs2, info1, info2, {cam1[0], cam1[1]}, {cam1[2], cam1[3]}, {cam2[0], cam2[1]}, {cam2[2], cam2[3]}, 0};
    s3x_sim3 inv;
    s3x_inverse(S, &inv);
    for (int i = 0; i < n; ++i) {
        double e12[2], e21[2];
        pair_errors(&p, i, S, &inv, e12, e21);
        out[2 * i] = edge_chi2(info1[i], e12); out[2 * i + 1] = edge_chi2(info2[i], e21);
    }
}

/* :1564-1624.  P1 / P2: s3x_prepare's output; info: mvInvLevelSigma2[octave] per pair.  kept [n]; cut_chi [2][n][2]: the chi2 the two
 * cuts compared (NaN where a pair was not looked at); est_out [3]: the initial estimate, the estimate after round 1, the last
 * tried estimate of the last round run. */
void s3x_optimize(const double *P1, const double *P2, const float *obs1, const float *obs2, const float *info1, const float *info2, int n,
                  const float cam1[4], const float cam2[4], const float R12[9], const float t12[3], float s12, float th2, int fix_scale,
                  s3x_result *res, uint8_t *kept, double *cut_chi, s3x_sim3 *est_out, s3x_trace *tr)
{
    prob_t p = {n, fix_scale, P1, P2, obs1, obs2, info1, info2, {cam1[0], cam1[1]}, {cam1[2], cam1[3]}, {cam2[0], cam2[1]}, {cam2[2], cam2[3]}, 0};
    const float deltaHuber = sqrtf(th2);                        /* :1479 */
    p.delta = deltaHuber;
    s3x_sim3 init, est, eval;
    s3x_from_rts(R12, t12, s12, &init);
    est = init; eval = init;
    memset(res, 0, sizeof(*res));
    if (tr) { memset(tr, 0, sizeof(*tr)); tr->min_abs_rho = INFINITY; }
    memcpy(res->q, init.q, sizeof(init.q)); memcpy(res->t, init.t, sizeof(init.t)); res->s = init.s;
    res->ncorrespondences = n;
    for (int i = 0; i < n; ++i) kept[i] = 1;
    if (cut_chi) for (int i = 0; i < 4 * n; ++i) cut_chi[i] = NAN;
    if (est_out) { est_out[0] = init; est_out[1] = init; est_out[2] = init; }
    if (n == 0) return;                                         /* no active vertex: optimize() returns -1 */
    run_round(&p, kept, &est, &eval, 5, &res->iterations[0], &res->trials[0], &res->chi2, tr, 0);
    if (est_out) { est_out[1] = est; est_out[2] = eval; }
    s3x_sim3 einv;
    s3x_inverse(&eval, &einv);
    int nBad = 0;
    for (int i = 0; i < n; ++i) {                               /* :1570-1587: _error is the last TRIED estimate's */
        double e12[2], e21[2];
        pair_errors(&p, i, &eval, &einv, e12, e21);
        const double a = edge_chi2(info1[i], e12), b = edge_chi2(info2[i], e21);
        if (cut_chi) { cut_chi[2 * i] = a; cut_chi[2 * i + 1] = b; }
        if (a > th2 || b > th2) { kept[i] = 0; nBad++; }
    }
    res->nbad = nBad;
    const int more = nBad > 0 ? 10 : 5;
    if (n - nBad < 10) return;                                  /* :1595: g2oS12 stays as it came in */
    run_round(&p, kept, &est, &eval, more, &res->iterations[1], &res->trials[1], &res->chi2, tr, 1);
    if (est_out) est_out[2] = eval;
    s3x_inverse(&eval, &einv);
    int nIn = 0;
    for (int i = 0; i < n; ++i) {                               /* :1604-1618 */
        if (!kept[i]) continue;
        double e12[2], e21[2];
        pair_errors(&p, i, &eval, &einv, e12, e21);
        const double a = edge_chi2(info1[i], e12), b = edge_chi2(info2[i], e21);
        if (cut_chi) { cut_chi[2 * n + 2 * i] = a; cut_chi[2 * n + 2 * i + 1] = b; }
        if (a > th2 || b > th2) kept[i] = 0;
        else nIn++;
    }
    res->nin = nIn;
    memcpy(res->q, est.q, sizeof(est.q)); memcpy(res->t, est.t, sizeof(est.t)); res->s = est.s;
}
