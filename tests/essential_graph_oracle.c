/* TEST INFRASTRUCTURE -- never part of the product.
 *
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1165-1428) restated for the CPU on the flattened graph of
 * include/orbslam_hip.h (orbm_eg_graph), independent of the library: it includes none of its headers, its loops run over run-time
 * dimensions, it keeps 3 x 3 matrices where the library keeps scalars, and its sums run in g2o's orders:
 *   computeActiveErrors / activeChi2   over the edges in edge order, ONE running sum
 *   buildSystem                        edge after edge: the numeric Jacobians (base_binary_edge.hpp:131-205), then A^T A and -A^T e into
 *                                      vertex 0's block, A^T B into the pair's block, B^T B and -B^T e into vertex 1's
 *   the solve                          a dense LLT of the lower triangle of H + lambda I in the caller's vertex order, every entry's dot
 *                                      from k = 0 upwards (tests/llt_reference.py's order; it stands in for LinearSolverEigen, as the
 *                                      library's does), then L y = b and L^T x = y
 *   update                             oplusImpl zeroes x[6] of the solver's vector when the scale is fixed
 *   computeScale                       one running sum over the whole update vector
 *   OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:63-241, bInFEA false; computeLambdaInit returns the
 *   user's value) and SparseOptimizer::optimize's loop with its break at the first result that is not OK.
 * A failed factorisation is a zero update and a rejected trial, as in the library.
 *
 * Test-only switch: ego_set_ulp(seed != 0) moves every sin / cos / acos / log / exp result by +1 or -1 ulp under a pattern of the
 * seed and the argument (exp(0) and log(1), exact in every libm, stay). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "g2o_restated.h"

typedef struct {
    int32_t nvert, ncorr, nnc, nedges, npoints, fix_scale;
    const float *poses;
    const int32_t *corrected;
    const double *corrected_sim3;
    const int32_t *noncorrected;
    const double *noncorrected_sim3;
    const uint8_t *fixed;
    const int32_t *e_v0, *e_v1;
    const uint8_t *e_kind;
    const float *points;
    const int32_t *p_ref;
} ego_graph;
typedef struct { int32_t iterations, reserved; double lambda_init; } ego_options;
typedef struct { double tempChi, currentChi, rho, lambda, scale; int32_t round, qmax, accepted, ok2; } ego_trial;
typedef struct {
    float *poses, *points;              /* [nvert][16], [npoints][3] */
    int32_t iterations, trials, nresults, results[64];
    int32_t trial_capacity, ntrials;
    ego_trial *trial_log;
    double *estimates, *chi2;           /* [nvert][8], [nedges] */
    double *J0, *b0;                    /* optional: [nedges][2][49] (row-major 7 x 7, error row by dimension) and [7 nact] of iteration 0 */
    double *meas;                       /* optional: [nedges][8] */
} ego_out;

typedef struct { double q[4], t[3], s; } sim3;

static uint64_t g_ulp;
void ego_set_ulp(uint64_t seed) { g_ulp = seed; }
/* v = f(arg) of a libm function moved by one ulp, up or down by a hash of the seed and the ARGUMENT's bits: another libm is still a
 * function, the same argument gives the same result.  (A pattern that runs on from call to call would give the two evaluations of a
 * numeric Jacobian column that the fixed scale makes identical different bits, and column 6 would no longer be exactly zero.) */
static double ulp(double v, double arg)
{
    if (!g_ulp) return v;
    uint64_t h;
    memcpy(&h, &arg, sizeof(h));
    h ^= g_ulp;
    h += 0x9e3779b97f4a7c15ull; h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull; h = (h ^ (h >> 27)) * 0x94d049bb133111ebull; h ^= h >> 31;
    return nextafter(v, (h >> 11) & 1 ? INFINITY : -INFINITY);
}

/* ---- 3 x 3 matrices, row-major */
static void m_skew(const double v[3], double m[9])
{
    memset(m, 0, 9 * sizeof(double));
    m[1] = -v[2]; m[2] = v[1]; m[5] = -v[0]; m[3] = v[2]; m[6] = -v[1]; m[7] = v[0];
}
static void m_mul(const double *a, const double *b, double *o)
{
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = a[3 * i] * b[j];
            for (int k = 1; k < 3; ++k) s = s + a[3 * i + k] * b[3 * k + j];
            r[3 * i + j] = s;
        }
    memcpy(o, r, sizeof(r));
}
static void q_to_matrix(const double q[4], double R[9])        /* Quaterniond::toRotationMatrix */
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

/* ---- types/sim3.h */
static void sim3_exp(const double u[7], sim3 *o)               /* Sim3(const Vector7d&) */
{
    const double sigma = u[6], theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double Om[9], O2[9], R[9], W[9], A, B, C;
    m_skew(u, Om);
    const double s = sigma == 0.0 ? 1.0 : ulp(exp(sigma), sigma);      /* exp(0) = 1 is exact in every libm */
    m_mul(Om, Om, O2);
    const double eps = 0.00001;
    const int small = theta < eps;
    double sn = 0, cs = 0;
    if (!small) { sn = ulp(sin(theta), theta); cs = ulp(cos(theta), theta); }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    for (int k = 0; k < 9; ++k) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        if (small) R[k] = I + Om[k] + O2[k];
        else R[k] = I + sn / theta * Om[k] + (1 - cs) / (theta * theta) * O2[k];
        W[k] = A * Om[k] + B * O2[k] + C * I;
    }
    quat_from_matrix(R, o->q);
    for (int i = 0; i < 3; ++i) o->t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o->s = s;
}
static void sim3_mul(const sim3 *A, const sim3 *B, sim3 *O)
{
    sim3 r;
    double rt[3];
    q_mul(A->q, B->q, r.q);
    q_rotate(A->q, B->t, rt);
    for (int k = 0; k < 3; ++k) r.t[k] = A->s * rt[k] + A->t[k];
    r.s = A->s * B->s;
    *O = r;
}
static void sim3_inverse(const sim3 *A, sim3 *O)
{
    sim3 r;
    const double f = -1. / A->s;
    double v[3];
    for (int k = 0; k < 3; ++k) { v[k] = f * A->t[k]; r.q[k] = -A->q[k]; }
    r.q[3] = A->q[3];
    q_rotate(r.q, v, r.t);
    r.s = 1. / A->s;
    *O = r;
}
static void sim3_map(const sim3 *S, const double X[3], double o[3])
{
    double r[3];
    q_rotate(S->q, X, r);
    for (int k = 0; k < 3; ++k) o[k] = S->s * r[k] + S->t[k];
}
/* Eigen's PartialPivLU of a 3 x 3 and its solve */
static void lu_solve(double *m, int n, const double *t, double *x)
{
    double y[8];
    for (int i = 0; i < n; ++i) y[i] = t[i];
    for (int k = 0; k < n; ++k) {
        int p = k;
        double big = fabs(m[n * k + k]);
        for (int i = k + 1; i < n; ++i)
            if (fabs(m[n * i + k]) > big) { big = fabs(m[n * i + k]); p = i; }
        if (p != k) {
            for (int c = 0; c < n; ++c) { const double s = m[n * k + c]; m[n * k + c] = m[n * p + c]; m[n * p + c] = s; }
            const double s = y[k]; y[k] = y[p]; y[p] = s;
        }
        if (big != 0.0)
            for (int i = k + 1; i < n; ++i) m[n * i + k] /= m[n * k + k];
        for (int i = k + 1; i < n; ++i)
            for (int c = k + 1; c < n; ++c) m[n * i + c] -= m[n * i + k] * m[n * k + c];
    }
    for (int i = 1; i < n; ++i) {
        double d = m[n * i] * y[0];
        for (int j = 1; j < i; ++j) d = d + m[n * i + j] * y[j];
        y[i] -= d;
    }
    for (int i = n - 1; i >= 0; --i) {
        if (i < n - 1) {
            double d = m[n * i + i + 1] * x[i + 1];
            for (int j = i + 2; j < n; ++j) d = d + m[n * i + j] * x[j];
            y[i] -= d;
        }
        x[i] = y[i] / m[n * i + i];
    }
}
void ego_sim3_log(const sim3 *S, double res[7])                /* Sim3::log */
{
    const double s = S->s, sigma = s == 1.0 ? 0.0 : ulp(log(s), s);  /* log(1) = 0 is exact in every libm */
    double R[9], omega[3], Om[9], BO[9], O2[9], W[9], A, B, C;
    q_to_matrix(S->q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta = ulp(acos(d), d), theta2 = theta * theta, f = theta / (2 * sqrt(1 - d * d));
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            A = (1 - ulp(cos(theta), theta)) / theta2;
            B = (theta - ulp(sin(theta), theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = ulp(acos(d), d), f = theta / (2 * sqrt(1 - d * d));
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            const double theta2 = theta * theta, a = s * ulp(sin(theta), theta), b = s * ulp(cos(theta), theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    m_skew(omega, Om);
    for (int k = 0; k < 9; ++k) BO[k] = B * Om[k];
    m_mul(BO, Om, O2);
    for (int k = 0; k < 9; ++k) W[k] = A * Om[k] + O2[k] + C * ((k % 4 == 0) ? 1.0 : 0.0);
    lu_solve(W, 3, S->t, res + 3);
    for (int k = 0; k < 3; ++k) res[k] = omega[k];
    res[6] = sigma;
}
void ego_sim3_exp(const double u[7], sim3 *o) { sim3_exp(u, o); }

static void edge_error(const sim3 *C, const sim3 *Si, const sim3 *Sj, double e[7])
{
    sim3 a, inv, err;
    sim3_mul(C, Si, &a);
    sim3_inverse(Sj, &inv);
    sim3_mul(&a, &inv, &err);
    ego_sim3_log(&err, e);
}
static void oplus(const sim3 *est, double *u, int fix_scale, sim3 *o)  /* VertexSim3Expmap::oplusImpl: writes into u */
{
    sim3 up;
    if (fix_scale) u[6] = 0;
    sim3_exp(u, &up);
    sim3_mul(&up, est, o);
}

/* the dense LLT of the lower triangle of the row-major S (n x n), in place; x = solution; returns ok.  Four entries of a row are
 * carried together (four independent running dots, each in ascending k: the order per entry is the contract's). */
static int llt_solve(double *S, int n, const double *b, double *x)
{
    for (int i = 0; i < n; ++i) {
        double *Li = S + (size_t)i * n;
        int j = 0;
        for (; j + 4 <= i; j += 4) {
            const double *L0 = S + (size_t)j * n, *L1 = L0 + n, *L2 = L1 + n, *L3 = L2 + n;
            double d[4] = {0, 0, 0, 0};
            if (j > 0) {
                d[0] = Li[0] * L0[0]; d[1] = Li[0] * L1[0]; d[2] = Li[0] * L2[0]; d[3] = Li[0] * L3[0];
                for (int k = 1; k < j; ++k) {
                    const double l = Li[k];
                    d[0] = d[0] + l * L0[k]; d[1] = d[1] + l * L1[k]; d[2] = d[2] + l * L2[k]; d[3] = d[3] + l * L3[k];
                }
            }
            for (int a = 0; a < 4; ++a) {
                const int jj = j + a;
                const double *Lj = S + (size_t)jj * n;
                double dot = d[a];
                int has = j > 0;
                for (int k = j; k < jj; ++k) {
                    if (has) dot = dot + Li[k] * Lj[k];
                    else { dot = Li[k] * Lj[k]; has = 1; }
                }
                Li[jj] = ((has ? Li[jj] - dot : Li[jj])) / Lj[jj];
            }
        }
        for (; j <= i; ++j) {
            const double *Lj = S + (size_t)j * n;
            double s = Li[j];
            if (j > 0) {
                double dot = Li[0] * Lj[0];
                for (int k = 1; k < j; ++k) dot = dot + Li[k] * Lj[k];
                s = s - dot;
            }
            if (i == j) {
                if (!(s > 0.0)) { for (int k = 0; k < n; ++k) x[k] = 0.0; return 0; }
                Li[j] = sqrt(s);
            } else
                Li[j] = s / Lj[j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double y = b[i];
        for (int j = 0; j < i; ++j) y -= S[(size_t)i * n + j] * x[j];
        x[i] = y / S[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double y = x[i];
        for (int j = n - 1; j > i; --j) y -= S[(size_t)j * n + i] * x[j];
        x[i] = y / S[(size_t)i * n + i];
    }
    return 1;
}

static void load(const double *a, int k, sim3 *S) { memcpy(S, a + 8 * (size_t)k, sizeof(sim3)); }

int ego_run(const ego_graph *g, const ego_options *opt, ego_out *out)
{
    const int nv = g->nvert, ne = g->nedges;
    sim3 *vScw = (sim3 *)calloc((size_t)nv + 1, sizeof(sim3)), *est = (sim3 *)calloc((size_t)nv + 1, sizeof(sim3));
    sim3 *bak = (sim3 *)calloc((size_t)nv + 1, sizeof(sim3)), *meas = (sim3 *)calloc((size_t)ne + 1, sizeof(sim3));
    double *err = (double *)calloc(7 * (size_t)ne + 1, sizeof(double));
    int *row = (int *)calloc((size_t)nv + 1, sizeof(int)), *cls = (int *)calloc((size_t)nv + 1, sizeof(int));
    for (int v = 0; v < nv; ++v) {                                  /* :1193-1228 */
        if (g->corrected[v] >= 0) load(g->corrected_sim3, g->corrected[v], &vScw[v]);
        else {
            const float *T = g->poses + 16 * (size_t)v;
            const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
            quat_from_matrix(R, vScw[v].q);
            vScw[v].t[0] = T[3]; vScw[v].t[1] = T[7]; vScw[v].t[2] = T[11];
            vScw[v].s = 1.0;
        }
        est[v] = vScw[v];
        cls[v] = g->fixed[v] ? 1 : 2;
    }
    for (int e = 0; e < ne; ++e) {                                  /* :1236-1367 */
        const int i = g->e_v0[e], j = g->e_v1[e];
        sim3 Siw = vScw[i], Sjw = vScw[j], Swi;
        if (g->e_kind[e]) {
            if (g->noncorrected[i] >= 0) load(g->noncorrected_sim3, g->noncorrected[i], &Siw);
            if (g->noncorrected[j] >= 0) load(g->noncorrected_sim3, g->noncorrected[j], &Sjw);
        }
        sim3_inverse(&Siw, &Swi);
        sim3_mul(&Sjw, &Swi, &meas[e]);
        if (out->meas) memcpy(out->meas + 8 * (size_t)e, &meas[e], sizeof(sim3));
        if (cls[i] == 2) cls[i] = 0;
        if (cls[j] == 2) cls[j] = 0;
    }
    int nact = 0;
    for (int v = 0; v < nv; ++v) row[v] = cls[v] == 0 ? nact++ : -1;
    const int n = 7 * nact, fs = g->fix_scale ? 1 : 0;
    out->iterations = 0; out->trials = 0; out->nresults = 0; out->ntrials = 0;

    if (ne > 0 && nact > 0 && opt->iterations > 0) {
        double *H = (double *)calloc((size_t)n * n, sizeof(double)), *S = (double *)calloc((size_t)n * n, sizeof(double));
        double *b = (double *)calloc((size_t)n, sizeof(double)), *x = (double *)calloc((size_t)n, sizeof(double));
        double lambda = 0, ni = 2, currentChi = 0;
        int nBad = 0, ok = 1;
        for (int it = 0; it < opt->iterations && ok; ++it) {
            /* computeActiveErrors, activeRobustChi2 */
            currentChi = 0;
            for (int e = 0; e < ne; ++e) {
                double *r = err + 7 * (size_t)e;
                edge_error(&meas[e], &est[g->e_v0[e]], &est[g->e_v1[e]], r);
                double c = r[0] * r[0];
                for (int k = 1; k < 7; ++k) c = c + r[k] * r[k];
                currentChi += c;
            }
            double tempChi = currentChi;
            const double iniChi = currentChi;
            /* buildSystem */
            memset(H, 0, sizeof(double) * (size_t)n * n);
            memset(b, 0, sizeof(double) * (size_t)n);
            for (int e = 0; e < ne; ++e) {
                const int v[2] = {g->e_v0[e], g->e_v1[e]};
                double J[2][49];
                memset(J, 0, sizeof(J));
                const double delta = 1e-9, scalar = 1.0 / (2 * delta);
                for (int side = 0; side < 2; ++side) {
                    if (cls[v[side]] == 1) continue;
                    double add[7] = {0, 0, 0, 0, 0, 0, 0};
                    for (int d = 0; d < 7; ++d) {
                        sim3 P;
                        double ep[7], em[7];
                        add[d] = delta;
                        oplus(&est[v[side]], add, fs, &P);
                        edge_error(&meas[e], side ? &est[v[0]] : &P, side ? &P : &est[v[1]], ep);
                        add[d] = -delta;
                        oplus(&est[v[side]], add, fs, &P);
                        edge_error(&meas[e], side ? &est[v[0]] : &P, side ? &P : &est[v[1]], em);
                        add[d] = 0.0;
                        for (int k = 0; k < 7; ++k) J[side][7 * k + d] = scalar * (ep[k] - em[k]);
                    }
                }
                if (it == 0 && out->J0) memcpy(out->J0 + 98 * (size_t)e, J, sizeof(J));
                const double *r = err + 7 * (size_t)e;
                for (int sa = 0; sa < 2; ++sa) {
                    if (cls[v[sa]] == 1) continue;
                    const int ra = 7 * row[v[sa]];
                    for (int p = 0; p < 7; ++p) {
                        double s = J[sa][p] * -r[0];
                        for (int k = 1; k < 7; ++k) s = s + J[sa][7 * k + p] * -r[k];
                        b[ra + p] += s;
                    }
                    for (int sb = sa; sb < 2; ++sb) {
                        if (cls[v[sb]] == 1) continue;
                        const int rb = 7 * row[v[sb]];
                        for (int p = 0; p < 7; ++p)
                            for (int q = 0; q < 7; ++q) {
                                double s = J[sa][p] * J[sb][q];
                                for (int k = 1; k < 7; ++k) s = s + J[sa][7 * k + p] * J[sb][7 * k + q];
                                if (sa == sb) H[(size_t)(ra + p) * n + ra + q] += s;
                                else if (rb > ra) H[(size_t)(rb + q) * n + ra + p] += s;    /* the lower triangle holds the transpose */
                                else H[(size_t)(ra + p) * n + rb + q] += s;
                            }
                    }
                }
            }
            if (it == 0) {
                lambda = opt->lambda_init; ni = 2; nBad = 0;
                if (out->b0) memcpy(out->b0, b, sizeof(double) * (size_t)n);
            }
            double rho = 0;
            int qmax = 0;
            do {
                memcpy(bak, est, sizeof(sim3) * (size_t)nv);                /* push */
                for (int i = 0; i < n; ++i) {
                    memcpy(S + (size_t)i * n, H + (size_t)i * n, sizeof(double) * (size_t)(i + 1));
                    S[(size_t)i * n + i] += lambda;
                }
                const int ok2 = llt_solve(S, n, b, x);
                for (int v = 0; v < nv; ++v) {
                    if (row[v] < 0) continue;
                    if (ok2) { sim3 o; oplus(&est[v], x + 7 * row[v], fs, &o); est[v] = o; }
                }
                tempChi = 0;
                for (int e = 0; e < ne; ++e) {
                    double *r = err + 7 * (size_t)e;
                    edge_error(&meas[e], &est[g->e_v0[e]], &est[g->e_v1[e]], r);
                    double c = r[0] * r[0];
                    for (int k = 1; k < 7; ++k) c = c + r[k] * r[k];
                    tempChi += c;
                }
                if (!ok2) tempChi = DBL_MAX;
                rho = currentChi - tempChi;
                double scale = 0;
                if (ok2) for (int j = 0; j < n; ++j) scale += x[j] * (lambda * x[j] + b[j]);
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
                    memcpy(est, bak, sizeof(sim3) * (size_t)nv);            /* pop */
                }
                if (out->ntrials < out->trial_capacity) {
                    ego_trial *t = &out->trial_log[out->ntrials];
                    t->tempChi = tempChi; t->currentChi = currentChi; t->rho = rho; t->lambda = lambda; t->scale = scale;
                    t->round = 0; t->qmax = qmax; t->accepted = good; t->ok2 = ok2;
                }
                out->ntrials++;
                qmax++;
            } while (rho < 0 && qmax < 10);
            out->iterations++;
            out->trials += qmax;
            int result;
            if (qmax == 10 || rho == 0) result = 2;
            else {
                if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
                else nBad = 0;
                result = nBad >= 3 ? 2 : 1;
            }
            if (out->nresults < 64) out->results[out->nresults] = result;
            out->nresults++;
            ok = result == 1;
        }
        free(H); free(S); free(b); free(x);
    }
    /* :1376-1427 */
    for (int v = 0; v < nv; ++v) {
        double R[9];
        q_to_matrix(est[v].q, R);
        const double f = 1. / est[v].s;
        float *o = out->poses + 16 * (size_t)v;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)R[3 * r + c];
            o[4 * r + 3] = (float)(est[v].t[r] * f);
        }
        o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 1;
        if (out->estimates) memcpy(out->estimates + 8 * (size_t)v, &est[v], sizeof(sim3));
    }
    for (int i = 0; i < g->npoints; ++i) {
        const int r = g->p_ref[i];
        sim3 Swr;
        sim3_inverse(&est[r], &Swr);
        const double P[3] = {g->points[3 * (size_t)i], g->points[3 * (size_t)i + 1], g->points[3 * (size_t)i + 2]};
        double a[3], c[3];
        sim3_map(&vScw[r], P, a);
        sim3_map(&Swr, a, c);
        for (int k = 0; k < 3; ++k) out->points[3 * (size_t)i + k] = (float)c[k];
    }
    for (int e = 0; e < ne && out->chi2; ++e) {
        const double *r = err + 7 * (size_t)e;
        double c = r[0] * r[0];
        for (int k = 1; k < 7; ++k) c = c + r[k] * r[k];
        out->chi2[e] = c;
    }
    free(vScw); free(est); free(bak); free(meas); free(err); free(row); free(cls);
    return 0;
}
