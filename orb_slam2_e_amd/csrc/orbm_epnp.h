// orbm_epnp.h -- EPnP as src/PnPsolver.cc:831-1457 has it and CheckInliers (:763-794), entirely in IEEE double (CheckInliers with
// the reference's own mix of float and double), written once for the host and the device.  Every step is + - * / sqrt, a
// comparison or a conversion: with -ffp-contract=off a device instantiation gives the bits of a host one.
//
// The OpenCV primitives are restated from OpenCV 3.4 (modules/core/src/lapack.cpp, matmul.cpp), unpinned like every OpenCV
// primitive of this project:
//   cvMulTransposed(.., 1)   every element (i, j >= i) is one double sum over the rows, k ascending from 0; the lower triangle is
//                            a copy of the upper
//   cvSVD(MODIFY_A | U_T)    JacobiSVDImpl_<double>: minval = DBL_MIN, eps = 10 DBL_EPSILON, at most max(m, 30) sweeps, the
//                            descending selection sort that swaps rows, the cv::RNG(0x12345678) tail; driven as _SVDcompute drives
//                            it for m >= n (the routine works on the transposed copy), Ut = the normalised rows.  Without U_T / V_T
//                            (estimate_R_and_t): u = the rows transposed, v = the transposed rotations.
//   cvInvert / cvSolve(CV_SVD)  the SVD, then SVBkSb with its threshold of 2 DBL_EPSILON times the sum of the singular values
// ONE departure from the reference: JacobiSVDImpl_<double> calls std::hypot, whose last bit differs between C libraries; here it
// is hypot_f64 below, the form of OpenCV's own JacobiImpl_ template.
// ONE place where the reference reads an indeterminate value: gauss_newton's x[4] when qr_solve returns early on a singular
// matrix in the first of the five iterations.  Here x starts as 0, and an early return leaves x as the previous iteration left it,
// as the reference does.
//
// Nothing is stored per correspondence.  The reference's alphas[i] and pcs[i] are pure functions of the correspondence and of a
// few doubles (cc_inv, cws[0]; ccs), so they are recomputed where they are read -- the same operations on the same operands give
// the same bits -- and solve_for_sign's negation of every pcs[i] is the negation of ccs, which the reference makes as well:
// rounding is symmetric, so -(a0 c0 + a1 c1 + a2 c2 + a3 c3) == a0 (-c0) + a1 (-c1) + a2 (-c2) + a3 (-c3) bit for bit.
//
// Work split: `Pol::each(count, f)` runs f(0) .. f(count - 1), each of which owns one output element (one whole sequential sum).
// The host policy is a loop; the device policy gives element e to lane e % 64 of the wave that runs the call, between two
// barriers.  Everything outside each() is computed by every lane from the same values (the Work arrays are in LDS on the device:
// every lane stores the same bits).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORBM_EPNP_HD __host__ __device__ __forceinline__
#else
#define ORBM_EPNP_HD inline
#endif

namespace orbm_epnp {

struct Serial {
    template <class F> ORBM_EPNP_HD void each(int count, F f) const { for (int e = 0; e < count; ++e) f(e); }
};

// The correspondences of one solve: sel == nullptr && mask == nullptr: 0 .. N-1; sel: the N listed ones (a minimal set, an index
// may repeat); mask: those i < N whose bit is set, in index order (Refine).  Coordinates are the solver's floats (mvP3Dw, mvP2D)
// widened as add_correspondence widens them, or doubles (the host test entry).
struct Points {
    const float *Xw = nullptr, *uv = nullptr;
    const double *pwd = nullptr, *usd = nullptr;
    const int32_t *sel = nullptr;
    const uint64_t *mask = nullptr;
    int N = 0, count = 0;               // count = number_of_correspondences
    ORBM_EPNP_HD bool has(int i) const { return !mask || ((mask[i >> 6] >> (i & 63)) & 1); }
    ORBM_EPNP_HD void pw(int i, double &x, double &y, double &z) const
    {
        const int k = sel ? sel[i] : i;
        if (pwd) { x = pwd[3 * k]; y = pwd[3 * k + 1]; z = pwd[3 * k + 2]; }
        else { x = (double)Xw[3 * k]; y = (double)Xw[3 * k + 1]; z = (double)Xw[3 * k + 2]; }
    }
    ORBM_EPNP_HD void us(int i, double &u, double &v) const
    {
        const int k = sel ? sel[i] : i;
        if (usd) { u = usd[2 * k]; v = usd[2 * k + 1]; }
        else { u = (double)uv[2 * k]; v = (double)uv[2 * k + 1]; }
    }
};

struct Work {
    double cws[4][3], ccs[4][3], ci[9];
    double ut[144], d[12];                       // MtM, then Ut of its SVD; the singular values
    double W[12], s0[12], s1[12];                // the Jacobi routine's squared norms and the staged products of its ordered sums
    double sa[30], sv[25], sw[5];                // At, Vt and w of the small decompositions
    double l_6x10[60], rho[6], dv[4][6][3], lk[30], bk[5];
    double betas[4], gn_a[24], gn_b[6], gn_x[4], A1[4], A2[4];
    double abt[9], pc0[3], pw0[3];
    double Rs[4][9], ts[4][3], rep[4];
};

ORBM_EPNP_HD double hypot_f64(double a, double b)
{
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

ORBM_EPNP_HD unsigned rng_next(uint64_t &state)     // cv::RNG::next(): multiply-with-carry
{
    state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
}

ORBM_EPNP_HD double ordered_sum(const double *s, int m)
{
    double r = 0;
    for (int k = 0; k < m; ++k) r += s[k];
    return r;
}

// JacobiSVDImpl_<double>(At, w, Vt, m, n, n1 = n, DBL_MIN, 10 DBL_EPSILON): At = n rows of length m, Vt = n x n.  want_vt = false
// leaves Vt alone (for a caller that reads only At and w: the rotations of Vt feed nothing else; the routine itself has a Vt
// whenever U or V is asked for, so rows are swapped and the tail runs either way).
template <class Pol>
ORBM_EPNP_HD void jacobi_svd(const Pol &pol, Work &wk, double *At, double *w, double *Vt, int m, int n, bool want_vt)
{
    const double eps = 2.220446049250313e-16 * 10, minval = 2.2250738585072014e-308;
    double *W = wk.W, *s0 = wk.s0, *s1 = wk.s1;
    for (int i = 0; i < n; ++i) {
        double *Ai = At + i * m;
        pol.each(m, [=](int k) { const double t = Ai[k]; s0[k] = t * t; });
        W[i] = ordered_sum(s0, m);
        if (want_vt)
            for (int k = 0; k < n; ++k) Vt[i * n + k] = i == k ? 1.0 : 0.0;
    }
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], p, b = W[j];
                pol.each(m, [=](int k) { s0[k] = Ai[k] * Aj[k]; });
                p = ordered_sum(s0, m);
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot_f64(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                pol.each(m, [=](int k) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    s0[k] = t0 * t0; s1[k] = t1 * t1;
                });
                W[i] = ordered_sum(s0, m); W[j] = ordered_sum(s1, m);
                changed = true;
                if (want_vt) {
                    double *Vi = Vt + i * n, *Vj = Vt + j * n;
                    pol.each(n, [=](int k) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    });
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double *Ai = At + i * m;
        pol.each(m, [=](int k) { const double t = Ai[k]; s0[k] = t * t; });
        W[i] = sqrt(ordered_sum(s0, m));
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            { const double t = W[i]; W[i] = W[j]; W[j] = t; }
            for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (want_vt)
                for (int k = 0; k < n; ++k) { const double t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    for (int i = 0; i < n; ++i) w[i] = W[i];
    uint64_t rng = 0x12345678;
    for (int i = 0; i < n; ++i) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            // a zero singular value: a random vector, the earlier rows projected out twice, normalised
            const double val0 = 1. / m;
            for (int k = 0; k < m; ++k) At[i * m + k] = (rng_next(rng) & 256) != 0 ? val0 : -val0;
            for (int it = 0; it < 2; ++it)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < m; ++k) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; ++k) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; ++k) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; sd += t * t; }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; ++k) At[i * m + k] *= s;
    }
}

// cvSolve(A, b, x, CV_SVD) of the 6 x nc system wk.lk (row-major) with b = wk.rho, into wk.bk: At = A.t(), JacobiSVD, then
// SVBkSb(m, n, w, u = At (uT), v = Vt (vT), b, nb = 1)
template <class Pol>
ORBM_EPNP_HD void solve_svd_6(const Pol &pol, Work &wk, int nc)
{
    const int m = 6;
    for (int r = 0; r < m; ++r)
        for (int c = 0; c < nc; ++c) wk.sa[c * m + r] = wk.lk[r * nc + c];
    jacobi_svd(pol, wk, wk.sa, wk.sw, wk.sv, m, nc, true);
    for (int j = 0; j < nc; ++j) wk.bk[j] = 0;
    double threshold = 0;
    for (int i = 0; i < nc; ++i) threshold += wk.sw[i];
    threshold *= 2.220446049250313e-16 * 2;
    for (int i = 0; i < nc; ++i) {
        double wi = wk.sw[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; ++j) s += wk.sa[i * m + j] * wk.rho[j];
        s *= wi;
        for (int j = 0; j < nc; ++j) wk.bk[j] = wk.bk[j] + s * wk.sv[i * nc + j];
    }
}

// cvInvert(CC, CC_inv, CV_SVD), 3 x 3: SVD::compute (u = At.t(), vt = Vt), then SVD::backSubst without a right-hand side
// (nb = m, buffer[j] = u[j][i] * (1 / w[i]), x[r][j] += vt[i][r] * buffer[j])
template <class Pol>
ORBM_EPNP_HD void invert_svd_3(const Pol &pol, Work &wk, const double *cc, double *inv)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) wk.sa[c * 3 + r] = cc[r * 3 + c];
    jacobi_svd(pol, wk, wk.sa, wk.sw, wk.sv, 3, 3, true);
    for (int k = 0; k < 9; ++k) inv[k] = 0;
    double threshold = 0;
    for (int i = 0; i < 3; ++i) threshold += wk.sw[i];
    threshold *= 2.220446049250313e-16 * 2;
    for (int i = 0; i < 3; ++i) {
        double wi = wk.sw[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double buffer[3];
        for (int j = 0; j < 3; ++j) buffer[j] = wk.sa[i * 3 + j] * wi;
        for (int r = 0; r < 3; ++r) {
            const double s = wk.sv[i * 3 + r];
            for (int j = 0; j < 3; ++j) inv[r * 3 + j] = inv[r * 3 + j] + s * buffer[j];
        }
    }
}

// alphas + 4 * i of compute_barycentric_coordinates (:880-891)
ORBM_EPNP_HD void alphas_of(const Work &wk, const Points &pts, int i, double &a0, double &a1, double &a2, double &a3)
{
    double x, y, z;
    pts.pw(i, x, y, z);
    const double *ci = wk.ci;
    const double dx = x - wk.cws[0][0], dy = y - wk.cws[0][1], dz = z - wk.cws[0][2];
    a1 = ci[0] * dx + ci[1] * dy + ci[2] * dz;
    a2 = ci[3] * dx + ci[4] * dy + ci[5] * dz;
    a3 = ci[6] * dx + ci[7] * dy + ci[8] * dz;
    a0 = 1.0 - a1 - a2 - a3;
}

// pcs + 3 * i of compute_pcs (:926-936), component j, from the current ccs
ORBM_EPNP_HD double pc_of(const Work &wk, const Points &pts, int i, int j)
{
    double a0, a1, a2, a3;
    alphas_of(wk, pts, i, a0, a1, a2, a3);
    return a0 * wk.ccs[0][j] + a1 * wk.ccs[1][j] + a2 * wk.ccs[2][j] + a3 * wk.ccs[3][j];
}

template <class Pol>
ORBM_EPNP_HD void choose_control_points(const Pol &pol, Work &wk, const Points &pts)
{
    Work *w = &wk;
    const Points *P = &pts;
    pol.each(3, [=](int j) {
        double s = 0;
        for (int i = 0; i < P->N; ++i) {
            if (!P->has(i)) continue;
            double p[3];
            P->pw(i, p[0], p[1], p[2]);
            s += j == 0 ? p[0] : j == 1 ? p[1] : p[2];
        }
        w->cws[0][j] = s / P->count;
    });
    // cvMulTransposed(PW0, PW0tPW0, 1): sa[9 ..] holds it, sa[0 .. 8] becomes its transposed copy
    double *ptp = wk.sa + 9;
    pol.each(6, [=](int e) {
        const int a = e < 3 ? 0 : e < 5 ? 1 : 2, b = e < 3 ? e : e < 5 ? e - 2 : 2;
        double s = 0;
        for (int i = 0; i < P->N; ++i) {
            if (!P->has(i)) continue;
            double p[3];
            P->pw(i, p[0], p[1], p[2]);
            const double pa = (a == 0 ? p[0] : a == 1 ? p[1] : p[2]) - w->cws[0][a], pb = (b == 0 ? p[0] : b == 1 ? p[1] : p[2]) - w->cws[0][b];
            s += pa * pb;
        }
        ptp[3 * a + b] = s;
    });
    ptp[3] = ptp[1]; ptp[6] = ptp[2]; ptp[7] = ptp[5];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) wk.sa[c * 3 + r] = ptp[r * 3 + c];
    jacobi_svd(pol, wk, wk.sa, wk.sw, wk.sv, 3, 3, false);          // dc = sw, uct = sa
    for (int i = 1; i < 4; ++i) {
        const double k = sqrt(wk.sw[i - 1] / pts.count);
        for (int j = 0; j < 3; ++j) wk.cws[i][j] = wk.cws[0][j] + k * wk.sa[3 * (i - 1) + j];
    }
}

template <class Pol>
ORBM_EPNP_HD void compute_barycentric_inverse(const Pol &pol, Work &wk)
{
    double cc[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 1; j < 4; ++j) cc[3 * i + j - 1] = wk.cws[j][i] - wk.cws[0][i];
    invert_svd_3(pol, wk, cc, wk.ci);
}

// fill_M of every correspondence and cvMulTransposed(M, MtM, 1): element (a, b >= a) adds the product of row 2 i, then that of
// row 2 i + 1, i ascending
template <class Pol>
ORBM_EPNP_HD void compute_mtm(const Pol &pol, Work &wk, const Points &pts, double fu, double fv, double uc, double vc)
{
    Work *w = &wk;
    const Points *P = &pts;
    pol.each(78, [=](int e) {
        int a = 0, rest = e;
        while (rest >= 12 - a) { rest -= 12 - a; ++a; }
        const int b = a + rest, ca = a / 3, ra = a % 3, cb = b / 3, rb = b % 3;
        double s = 0;
        for (int i = 0; i < P->N; ++i) {
            if (!P->has(i)) continue;
            double as[4], u, v;
            alphas_of(*w, *P, i, as[0], as[1], as[2], as[3]);
            P->us(i, u, v);
            const double aa = ca == 0 ? as[0] : ca == 1 ? as[1] : ca == 2 ? as[2] : as[3];
            const double ab = cb == 0 ? as[0] : cb == 1 ? as[1] : cb == 2 ? as[2] : as[3];
            const double m1a = ra == 0 ? aa * fu : ra == 1 ? 0.0 : aa * (uc - u), m1b = rb == 0 ? ab * fu : rb == 1 ? 0.0 : ab * (uc - u);
            const double m2a = ra == 0 ? 0.0 : ra == 1 ? aa * fv : aa * (vc - v), m2b = rb == 0 ? 0.0 : rb == 1 ? ab * fv : ab * (vc - v);
            s += m1a * m1b;
            s += m2a * m2b;
        }
        w->ut[12 * a + b] = s;
    });
    for (int a = 1; a < 12; ++a)
        for (int b = 0; b < a; ++b) wk.ut[12 * a + b] = wk.ut[12 * b + a];
}

ORBM_EPNP_HD double dot3(const double *v1, const double *v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }
ORBM_EPNP_HD double dist2(const double *p1, const double *p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

ORBM_EPNP_HD void compute_L_6x10_and_rho(Work &wk)
{
    for (int i = 0; i < 4; ++i) {
        const double *v = wk.ut + 12 * (11 - i);
        int a = 0, b = 1;
        for (int j = 0; j < 6; ++j) {
            wk.dv[i][j][0] = v[3 * a] - v[3 * b];
            wk.dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
            wk.dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; ++i) {
        double *row = wk.l_6x10 + 10 * i;
        row[0] = dot3(wk.dv[0][i], wk.dv[0][i]);
        row[1] = 2.0 * dot3(wk.dv[0][i], wk.dv[1][i]);
        row[2] = dot3(wk.dv[1][i], wk.dv[1][i]);
        row[3] = 2.0 * dot3(wk.dv[0][i], wk.dv[2][i]);
        row[4] = 2.0 * dot3(wk.dv[1][i], wk.dv[2][i]);
        row[5] = dot3(wk.dv[2][i], wk.dv[2][i]);
        row[6] = 2.0 * dot3(wk.dv[0][i], wk.dv[3][i]);
        row[7] = 2.0 * dot3(wk.dv[1][i], wk.dv[3][i]);
        row[8] = 2.0 * dot3(wk.dv[2][i], wk.dv[3][i]);
        row[9] = dot3(wk.dv[3][i], wk.dv[3][i]);
    }
    wk.rho[0] = dist2(wk.cws[0], wk.cws[1]);
    wk.rho[1] = dist2(wk.cws[0], wk.cws[2]);
    wk.rho[2] = dist2(wk.cws[0], wk.cws[3]);
    wk.rho[3] = dist2(wk.cws[1], wk.cws[2]);
    wk.rho[4] = dist2(wk.cws[1], wk.cws[3]);
    wk.rho[5] = dist2(wk.cws[2], wk.cws[3]);
}

// find_betas_approx_1 / _2 / _3 (:1138-1241)
template <class Pol>
ORBM_EPNP_HD void find_betas_approx(const Pol &pol, Work &wk, int which)
{
    const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
    for (int i = 0; i < 6; ++i)
        for (int c = 0; c < nc; ++c) {
            const int col = which == 1 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c;
            wk.lk[i * nc + c] = wk.l_6x10[10 * i + col];
        }
    solve_svd_6(pol, wk, nc);
    const double *b = wk.bk;
    double *betas = wk.betas;
    if (which == 1) {
        if (b[0] < 0) {
            betas[0] = sqrt(-b[0]);
            betas[1] = -b[1] / betas[0];
            betas[2] = -b[2] / betas[0];
            betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = sqrt(b[0]);
            betas[1] = b[1] / betas[0];
            betas[2] = b[2] / betas[0];
            betas[3] = b[3] / betas[0];
        }
        return;
    }
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
}

// qr_solve (:1349-1455) of the 6 x 4 system gn_a, gn_b into gn_x; false = the singular-matrix early return (gn_x untouched)
ORBM_EPNP_HD bool qr_solve_6x4(Work &wk)
{
    const int nr = 6, nc = 4;
    double *pA = wk.gn_a, *pb = wk.gn_b, *pX = wk.gn_x, *A1 = wk.A1, *A2 = wk.A2;
    for (int k = 0; k < nc; ++k) {
        double eta = fabs(pA[k * nc + k]);
        // the reference's scan starts at i = k + 1 but reads the element of row i - 1 (its pointer advances after the read)
        for (int i = k + 1; i < nr; ++i) {
            const double elt = fabs(pA[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return false;
        }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; ++i) {
            pA[i * nc + k] *= inv_eta;
            sum += pA[i * nc + k] * pA[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (pA[k * nc + k] < 0) sigma = -sigma;
        pA[k * nc + k] += sigma;
        A1[k] = sigma * pA[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s = 0;
            for (int i = k; i < nr; ++i) s += pA[i * nc + k] * pA[i * nc + j];
            const double tau = s / A1[k];
            for (int i = k; i < nr; ++i) pA[i * nc + j] -= tau * pA[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {                          // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau += pA[i * nc + j] * pb[i];
        tau /= A1[j];
        for (int i = j; i < nr; ++i) pb[i] -= tau * pA[i * nc + j];
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];                   // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) sum += pA[i * nc + j] * pX[j];
        pX[i] = (pb[i] - sum) / A2[i];
    }
    return true;
}

ORBM_EPNP_HD void gauss_newton(Work &wk)
{
    double *betas = wk.betas;
    for (int i = 0; i < 4; ++i) wk.gn_x[i] = 0;
    for (int k = 0; k < 5; ++k) {
        for (int i = 0; i < 6; ++i) {
            const double *rowL = wk.l_6x10 + i * 10;
            double *rowA = wk.gn_a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            wk.gn_b[i] = wk.rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                                      rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                                      rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                                      rowL[9] * betas[3] * betas[3]);
        }
        qr_solve_6x4(wk);
        for (int i = 0; i < 4; ++i) betas[i] += wk.gn_x[i];
    }
}

// compute_R_and_t (:1122-1133): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
template <class Pol>
ORBM_EPNP_HD double compute_R_and_t(const Pol &pol, Work &wk, const Points &pts, double fu, double fv, double uc, double vc, double *R, double *t)
{
    Work *w = &wk;
    const Points *P = &pts;
    for (int i = 0; i < 4; ++i) wk.ccs[i][0] = wk.ccs[i][1] = wk.ccs[i][2] = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double *v = wk.ut + 12 * (11 - i);
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 3; ++k) wk.ccs[j][k] += wk.betas[i] * v[3 * j + k];
    }
    int first = 0;
    while (first < pts.N && !pts.has(first)) ++first;
    if (pc_of(wk, pts, first, 2) < 0.0)                     // solve_for_sign: pcs[2] is the z of the first correspondence
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 3; ++j) wk.ccs[i][j] = -wk.ccs[i][j];
    // estimate_R_and_t
    pol.each(6, [=](int e) {
        const int j = e % 3;
        double s = 0.0;
        for (int i = 0; i < P->N; ++i) {
            if (!P->has(i)) continue;
            if (e < 3) s += pc_of(*w, *P, i, j);
            else {
                double p[3];
                P->pw(i, p[0], p[1], p[2]);
                s += j == 0 ? p[0] : j == 1 ? p[1] : p[2];
            }
        }
        (e < 3 ? w->pc0 : w->pw0)[j] = s / P->count;
    });
    pol.each(9, [=](int e) {
        const int j = e / 3, c = e % 3;
        double s = 0.0;
        for (int i = 0; i < P->N; ++i) {
            if (!P->has(i)) continue;
            double p[3];
            P->pw(i, p[0], p[1], p[2]);
            s += (pc_of(*w, *P, i, j) - w->pc0[j]) * ((c == 0 ? p[0] : c == 1 ? p[1] : p[2]) - w->pw0[c]);
        }
        w->abt[e] = s;
    });
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) wk.sa[c * 3 + r] = wk.abt[r * 3 + c];
    jacobi_svd(pol, wk, wk.sa, wk.sw, wk.sv, 3, 3, true);
    // abt_u[i][k] = sa[k][i], abt_v[j][k] = sv[k][j]
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = wk.sa[i] * wk.sv[j] + wk.sa[3 + i] * wk.sv[3 + j] + wk.sa[6 + i] * wk.sv[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    t[0] = wk.pc0[0] - dot3(R, wk.pw0);
    t[1] = wk.pc0[1] - dot3(R + 3, wk.pw0);
    t[2] = wk.pc0[2] - dot3(R + 6, wk.pw0);
    // reprojection_error
    double sum2 = 0.0;
    for (int i = 0; i < pts.N; ++i) {
        if (!pts.has(i)) continue;
        double pw[3], u, v;
        pts.pw(i, pw[0], pw[1], pw[2]);
        pts.us(i, u, v);
        const double Xc = dot3(R, pw) + t[0], Yc = dot3(R + 3, pw) + t[1], inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
        const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / pts.count;
}

// compute_pose (:938-986): R[9] row-major, t[3]; returns rep_errors[N]
template <class Pol>
ORBM_EPNP_HD double compute_pose(const Pol &pol, Work &wk, const Points &pts, double fu, double fv, double uc, double vc, double *R, double *t)
{
    choose_control_points(pol, wk, pts);
    compute_barycentric_inverse(pol, wk);
    compute_mtm(pol, wk, pts, fu, fv, uc, vc);
    // cvSVD(MtM, D, Ut, 0, MODIFY_A | U_T): the routine's At is MtM.t(), and MtM's lower triangle is a copy of its upper
    jacobi_svd(pol, wk, wk.ut, wk.d, wk.sv, 12, 12, false);
    compute_L_6x10_and_rho(wk);
    for (int which = 1; which <= 3; ++which) {
        find_betas_approx(pol, wk, which);
        gauss_newton(wk);
        wk.rep[which] = compute_R_and_t(pol, wk, pts, fu, fv, uc, vc, wk.Rs[which], wk.ts[which]);
    }
    int N = 1;
    if (wk.rep[2] < wk.rep[1]) N = 2;
    if (wk.rep[3] < wk.rep[N]) N = 3;
    for (int k = 0; k < 9; ++k) R[k] = wk.Rs[N][k];
    for (int k = 0; k < 3; ++k) t[k] = wk.ts[N][k];
    return wk.rep[N];
}

// One correspondence of CheckInliers (:767-792) with the reference's types: double row sums narrowed to float, invZc = the float
// of 1 / (double sum), ue / ve in double, float differences, a float sum of float squares, strict < against mvMaxError[i]
ORBM_EPNP_HD bool check_inlier(const double *R, const double *t, const float *X, const float *p2d, double fu, double fv, double uc, double vc,
                               float max_error)
{
    const float Xc = (float)(R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]);
    const float Yc = (float)(R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]));
    const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
    const float distX = (float)(p2d[0] - ue), distY = (float)(p2d[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}

} // namespace orbm_epnp
