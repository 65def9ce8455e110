/* TEST INFRASTRUCTURE -- never part of the product.
 *
 * What the two g2o restatements (tests/pose_only_oracle.c, tests/sim3_opt_oracle.c) share of Eigen 3.3, restated once: the
 * quaternion constructor, product and rotation, and the pivoting LDLT of LinearSolverDense.  The device code has the same slice in
 * orb_slam2_e_amd/csrc/orbm_g2o_math.h.  Every function tolerates an output that aliases an input. */
#ifndef G2O_RESTATED_H
#define G2O_RESTATED_H
#include <math.h>
#include <string.h>

/* Quaterniond(const Matrix3d&) (Eigen quaternionbase_assign_substitute_pair), R row major, q = x y z w: not normalised */
static void quat_from_matrix(const double R[9], double q[4])
{
#define M(i, j) R[3 * (i) + (j)]
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (M(2, 1) - M(1, 2)) * t;
        q[1] = (M(0, 2) - M(2, 0)) * t;
        q[2] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (M(k, j) - M(j, k)) * t;
        q[j] = (M(j, i) + M(i, j)) * t;
        q[k] = (M(k, i) + M(i, k)) * t;
    }
#undef M
}

/* Quaternion product a * b (Eigen quat_product) */
static void q_mul(const double a[4], const double b[4], double o[4])
{
    double r[4];
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    memcpy(o, r, sizeof(r));
}

/* Quaternion * Vector3d (Eigen _transformVector): uv = vec x v; uv += uv; v + w uv + vec x uv */
static void q_rotate(const double q[4], const double v[3], double o[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = v[i] + q[3] * uv[i] + c[i];
    memcpy(o, r, sizeof(r));
}

/* What ldlt_solve does when no diagonal entry is > 0 in magnitude at step 0 -- an all-zero diagonal, or a matrix of NaN:
 *   LDLT_AS_EIGEN     Eigen's "the entire diagonal is zero" exit: ZeroSign, identity transpositions, the matrix as it is, and the
 *                     solve runs on it.  A zero matrix gives x = 0 (D^-1 = 0), a NaN matrix x = NaN.  sim3_opt_oracle.c uses it.
 *   LDLT_RETURN_ZERO  x = 0 and isPositive() at once: the same for a zero matrix, but x = 0 for a NaN matrix too.
 *                     pose_only_oracle.c uses it.
 * Both restatements keep the behaviour their device kernels were written against (LdltZeroDiagonal in orbm_g2o_math.h). */
enum { LDLT_AS_EIGEN = 0, LDLT_RETURN_ZERO = 1 };

/* Eigen::LDLT<MatrixXd> (ldlt_inplace, Eigen 3.3: diagonal pivoting on the lower triangle) of the n x n (n <= 7) row-major m, in
 * place, then solve(b) and isPositive() (linear_solver_dense.h:104-110).  Returns isPositive(); x is written only then. */
static int ldlt_solve(double *m, const double *b, int n, int zero_diagonal, double *x)
{
    int tr[7], sign = 0;   /* 0 ZeroSign, 1 PositiveSemiDef, 2 NegativeSemiDef, 3 Indefinite */
    double temp[7];
#define L(i, j) m[(i) * n + (j)]
    for (int k = 0; k < n; ++k) {
        int big = k;                                   /* diagonal().tail(n-k).cwiseAbs().maxCoeff(&index) */
        double bv = fabs(L(k, k));
        for (int j = k + 1; j < n; ++j) {
            const double f = fabs(L(j, j));
            if (f > bv) { big = j; bv = f; }
        }
        tr[k] = big;
        if (big != k) {
            const int c = big;
            for (int j = 0; j < k; ++j) { const double s = L(k, j); L(k, j) = L(c, j); L(c, j) = s; }
            for (int i = c + 1; i < n; ++i) { const double s = L(i, k); L(i, k) = L(i, c); L(i, c) = s; }
            { const double s = L(k, k); L(k, k) = L(c, c); L(c, c) = s; }
            for (int i = k + 1; i < c; ++i) { const double s = L(i, k); L(i, k) = L(c, i); L(c, i) = s; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) temp[j] = L(j, j) * L(k, j);
            double s = L(k, 0) * temp[0];
            for (int j = 1; j < k; ++j) s = s + L(k, j) * temp[j];
            L(k, k) -= s;
            for (int i = k + 1; i < n; ++i) {
                double a = L(i, 0) * temp[0];
                for (int j = 1; j < k; ++j) a = a + L(i, j) * temp[j];
                L(i, k) -= a;
            }
        }
        const double akk = L(k, k);
        const int valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            if (zero_diagonal == LDLT_RETURN_ZERO) { for (int j = 0; j < n; ++j) x[j] = 0.0; return 1; }
            for (int j = 0; j < n; ++j) tr[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < n; ++i) L(i, k) /= akk;
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return 0;
    /* LDLT::solve: x = P b; L^-1; D^-1 (|d| > DBL_MIN, else 0); L^-T; P^T */
    double y[7];
    for (int i = 0; i < n; ++i) y[i] = b[i];
    for (int k = 0; k < n; ++k) if (tr[k] != k) { const double s = y[k]; y[k] = y[tr[k]]; y[tr[k]] = s; }
    for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) y[i] -= L(i, j) * y[j];
    for (int i = 0; i < n; ++i) y[i] = (fabs(L(i, i)) > 2.2250738585072014e-308) ? y[i] / L(i, i) : 0.0;
    for (int i = n - 1; i >= 0; --i) for (int j = i + 1; j < n; ++j) y[i] -= L(j, i) * y[j];
    for (int k = n - 1; k >= 0; --k) if (tr[k] != k) { const double s = y[k]; y[k] = y[tr[k]]; y[tr[k]] = s; }
    for (int i = 0; i < n; ++i) x[i] = y[i];
#undef L
    return 1;
}

#endif
