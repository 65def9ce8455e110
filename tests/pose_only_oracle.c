/* TEST INFRASTRUCTURE -- never part of the product, never linked into liborbslam_hip.so.
 *
 * A literal restatement of Optimizer::PoseOptimization (src/Optimizer.cc:264-476) on the code paths g2o takes for it: one
 * VertexSE3Expmap, N unary EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose edges with Huber kernels,
 * BlockSolver_6_3 over LinearSolverDense, OptimizationAlgorithmLevenberg, 4 rounds x 10 iterations with the inlier / outlier
 * reclassification between rounds.  Plain C99, double throughout (float where the reference has float).  Each function names the
 * reference lines it follows (Thirdparty/g2o/g2o/...); the few Eigen routines involved are restated and named where used, those the
 * OptimizeSim3 restatement needs too in tests/g2o_restated.h.
 * tests/pose_only_oracle.py compiles this file and wraps it with ctypes; the device kernel (orbm_pose.hip) is checked against it.
 *
 * Sums over edges run in edge order (= keypoint order: SparseOptimizer::sortVectorContainers sorts _activeEdges by id,
 * sparse_optimizer.cpp:567-572, and the edges are added in keypoint order). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "g2o_restated.h"

typedef struct { double q[4]; double t[3]; } po_se3;   /* q = x y z w (Eigen's coeffs() order) */

typedef struct {
    int32_t rounds, iterations[4], trials[4], ninitial;
    double chi2, q[4], t[3];
    /* restatement only: how close the discrete decisions came to flipping */
    double min_rho;        /* min |rho| over all accept / reject decisions (rho / scale, optimization_algorithm_levenberg.cpp:211) */
    double min_class;      /* min |chi2 - th| / th over all classifications (Optimizer.cc:405, :434), on the float chi2 */
    double min_stop;       /* min |(iniChi - currentChi) * 1e3 - iniChi| / iniChi (Raul's stop criterion, levenberg.cpp:236) */
    double round_chi2[4];  /* each round's last currentChi */
    double chi2_plain[4], chi2_robust[4];   /* at each round's final estimate, over its active edges: plain / Huber chi2 */
} po_stats;

/* ---------------------------------------------------------------- Eigen / se3quat.h restated */

/* Quaterniond::normalize (Eigen: q /= sqrt(squaredNorm()), coefficients x y z w) */
static void q_normalize(double q[4])
{
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n > 0.0) {
        const double s = sqrt(n);
        q[0] /= s; q[1] /= s; q[2] /= s; q[3] /= s;
    }
}

/* SE3Quat::normalizeRotation (se3quat.h): w >= 0, unit norm */
static void normalize_rotation(double q[4])
{
    if (q[3] < 0) { q[0] *= -1; q[1] *= -1; q[2] *= -1; q[3] *= -1; }
    q_normalize(q);
}

/* Quaterniond(const Matrix3d&), R row major (tests/g2o_restated.h, as the quaternion product and rotation below) */
void po_quat_from_matrix(const double R[9], double q[4]) { quat_from_matrix(R, q); }

/* QuaternionBase::toRotationMatrix (Eigen), R row major */
void po_quat_to_matrix(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

/* SE3Quat::map (se3quat.h): r * xyz + t */
void po_map(const po_se3 *T, const double X[3], double o[3])
{
    q_rotate(T->q, X, o);
    o[0] += T->t[0]; o[1] += T->t[1]; o[2] += T->t[2];
}

static void mat3_mul(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

/* SE3Quat::exp (se3quat.h), update = (omega, upsilon); skew() of se3_ops.hpp */
void po_exp(const double u[6], po_se3 *T)
{
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);   /* Vector3d::norm */
    const double Om[9] = {0., -w2, w1, w2, 0., -w0, -w1, w0, 0.};
    double O2[9], R[9], V[9];
    mat3_mul(Om, Om, O2);
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
        memcpy(V, R, sizeof(R));
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / (pow(theta, 3));
        for (int k = 0; k < 9; ++k) {
            const double I = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = I + a * Om[k] + b * O2[k];
            V[k] = I + b * Om[k] + c * O2[k];
        }
    }
    po_quat_from_matrix(R, T->q);
    for (int i = 0; i < 3; ++i) T->t[i] = V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
    normalize_rotation(T->q);          /* SE3Quat(const Quaterniond&, const Vector3d&) */
}

/* SE3Quat::operator*(const SE3Quat&) (se3quat.h) */
void po_compose(const po_se3 *A, const po_se3 *B, po_se3 *O)
{
    po_se3 r = *A;
    double rt[3];
    q_rotate(A->q, B->t, rt);
    r.t[0] += rt[0]; r.t[1] += rt[1]; r.t[2] += rt[2];
    q_mul(A->q, B->q, r.q);
    normalize_rotation(r.q);
    *O = r;
}

/* Converter::toSE3Quat (src/Converter.cc:37-47): float 4x4 row major -> SE3Quat(Matrix3d, Vector3d) */
void po_from_cv(const float T[16], po_se3 *o)
{
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    po_quat_from_matrix(R, o->q);
    o->t[0] = T[3]; o->t[1] = T[7]; o->t[2] = T[11];
    normalize_rotation(o->q);
}

/* Converter::toCvMat(const SE3Quat&) (src/Converter.cc:49-71, to_homogeneous_matrix) */
void po_to_cv(const po_se3 *s, float T[16])
{
    double R[9];
    po_quat_to_matrix(s->q, R);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
        T[4 * i + 3] = (float)s->t[i];
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

/* LinearSolverDense's LDLT of the n x n (n <= 6) row-major A (A is not changed); x = 0 where the diagonal has no entry to pivot on */
int po_ldlt_solve(const double *A, const double *b, int n, double *x)
{
    double m[36];
    memcpy(m, A, sizeof(double) * n * n);
    return ldlt_solve(m, b, n, LDLT_RETURN_ZERO, x);
}

/* ---------------------------------------------------------------- the edges (types_six_dof_expmap.h:196-260, .cpp:266-364) */

typedef struct {
    double obs[3], Xw[3], info;    /* measurement, Xw, information = invSigma2 * I (all from floats) */
    int stereo, kp;                /* edge kind, keypoint index */
    int level, robust;             /* setLevel, robust kernel attached */
    double err[3];                 /* _error as the last computeError left it */
    int level_r4, pad;             /* the level during round 4 (0: one of its active edges; set only when round 4 runs) */
} po_edge;

typedef struct { double fx, fy, cx, cy, bf; } po_cam;

/* EdgeSE3ProjectXYZOnlyPose::computeError / EdgeStereoSE3ProjectXYZOnlyPose::computeError with cam_project (.cpp:306-325) */
void po_edge_error(const po_cam *c, int stereo, const double obs[3], const double Xw[3], const po_se3 *T, double err[3])
{
    double p[3];
    po_map(T, Xw, p);
    if (!stereo) {
        const double u = p[0] / p[2], v = p[1] / p[2];          /* project2d */
        err[0] = obs[0] - (u * c->fx + c->cx);
        err[1] = obs[1] - (v * c->fy + c->cy);
        err[2] = 0.0;
    } else {
        const float invz = 1.0f / p[2];                          /* float, as cam_project(trans_xyz) of the stereo edge */
        const double r0 = p[0] * invz * c->fx + c->cx;
        const double r1 = p[1] * invz * c->fy + c->cy;
        const double r2 = r0 - c->bf * invz;
        err[0] = obs[0] - r0; err[1] = obs[1] - r1; err[2] = obs[2] - r2;
    }
}

/* linearizeOplus of both edges (.cpp:266-290, :342-364): J row major [3][6] (third row: stereo only) */
void po_edge_jacobian(const po_cam *c, int stereo, const double Xw[3], const po_se3 *T, double J[18])
{
    double p[3];
    po_map(T, Xw, p);
    const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
    J[0] = x * y * invz_2 * c->fx; J[1] = -(1 + (x * x * invz_2)) * c->fx; J[2] = y * invz * c->fx;
    J[3] = -invz * c->fx;          J[4] = 0;                                J[5] = x * invz_2 * c->fx;
    J[6] = (1 + y * y * invz_2) * c->fy; J[7] = -x * y * invz_2 * c->fy; J[8] = -x * invz * c->fy;
    J[9] = 0;                            J[10] = -invz * c->fy;          J[11] = y * invz_2 * c->fy;
    if (stereo) {
        J[12] = J[0] - c->bf * y * invz_2; J[13] = J[1] + c->bf * x * invz_2; J[14] = J[2];
        J[15] = J[3];                      J[16] = 0;                         J[17] = J[5] - c->bf * invz_2;
    } else {
        for (int k = 12; k < 18; ++k) J[k] = 0;
    }
}

/* BaseEdge::chi2 = _error.dot(information() * _error), information diagonal (off-diagonal zeros multiplied, as Eigen does) */
static double edge_chi2(const po_edge *e)
{
    const int D = e->stereo ? 3 : 2;
    double oe[3];
    for (int i = 0; i < D; ++i) {
        double s = ((i == 0) ? e->info : 0.0) * e->err[0];
        for (int j = 1; j < D; ++j) s += ((i == j) ? e->info : 0.0) * e->err[j];
        oe[i] = s;
    }
    double r = e->err[0] * oe[0];
    for (int i = 1; i < D; ++i) r += e->err[i] * oe[i];
    return r;
}

/* RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:60-80): dsqr is a FLOAT member (robust_kernel_impl.h:84) */
static void huber(double e, double delta, double rho[3])
{
    const float dsqr = (float)(delta * delta);
    if (e <= dsqr) { rho[0] = e; rho[1] = 1.; rho[2] = 0.; }
    else {
        const double sqrte = sqrt(e);
        rho[0] = 2 * sqrte * delta - dsqr;
        rho[1] = delta / sqrte;
        rho[2] = -0.5 * rho[1] / e;
    }
}

/* ---------------------------------------------------------------- the optimizer */

typedef struct {
    po_edge *e;
    int ne;
    po_cam cam;
    double delta_mono, delta_stereo;
    po_se3 est;
    double H[36], b[6];
} po_graph;

/* SparseOptimizer::computeActiveErrors (sparse_optimizer.cpp:60-113) */
static void compute_active_errors(po_graph *g)
{
    for (int k = 0; k < g->ne; ++k)
        if (g->e[k].level == 0) po_edge_error(&g->cam, g->e[k].stereo, g->e[k].obs, g->e[k].Xw, &g->est, g->e[k].err);
}

/* SparseOptimizer::activeRobustChi2 (sparse_optimizer.cpp:169-186) */
static double active_robust_chi2(const po_graph *g)
{
    double chi = 0.0;
    for (int k = 0; k < g->ne; ++k) {
        const po_edge *e = &g->e[k];
        if (e->level != 0) continue;
        if (e->robust) {
            double rho[3];
            huber(edge_chi2(e), e->stereo ? g->delta_stereo : g->delta_mono, rho);
            chi += rho[0];
        } else chi += edge_chi2(e);
    }
    return chi;
}

/* BlockSolver::buildSystem (block_solver.hpp:512-562) with BaseUnaryEdge::constructQuadraticForm (base_unary_edge.hpp:40-70) and
 * robustInformation (base_edge.h:96-102: rho[1] * information; the rho[2] term is commented out) */
static void build_system(po_graph *g)
{
    memset(g->H, 0, sizeof(g->H));
    memset(g->b, 0, sizeof(g->b));
    for (int k = 0; k < g->ne; ++k) {
        const po_edge *e = &g->e[k];
        if (e->level != 0) continue;
        const int D = e->stereo ? 3 : 2;
        double J[18];
        po_edge_jacobian(&g->cam, e->stereo, e->Xw, &g->est, J);
        double w = 1.0;
        if (e->robust) {
            double rho[3];
            huber(edge_chi2(e), e->stereo ? g->delta_stereo : g->delta_mono, rho);
            w = rho[1];
        }
        const double winfo = w * e->info;         /* weightedOmega (diagonal); plain omega when w = 1 */
        for (int r = 0; r < 6; ++r) {
            double s = 0;                          /* (A^T omega e)_r */
            for (int i = 0; i < D; ++i) s += J[6 * i + r] * (e->info * e->err[i]);
            g->b[r] -= w * s;
            for (int c = 0; c < 6; ++c) {
                double h = 0;
                for (int i = 0; i < D; ++i) h += J[6 * i + r] * (winfo * J[6 * i + c]);
                g->H[6 * r + c] += h;
            }
        }
    }
}

/* OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:63-240) with its state */
typedef struct { double lambda; int ni, nBad, trials; double currentChi; } po_lm;
enum { PO_OK = 0, PO_TERMINATE = 1 };

static void track_min(double *m, double v) { if (v < *m) *m = v; }   /* minimum of |margins|, NaN ignored */

static int lm_solve(po_graph *g, po_lm *lm, int iteration, po_stats *st)
{
    compute_active_errors(g);
    double currentChi = active_robust_chi2(g);
    double tempChi = currentChi;
    const double iniChi = currentChi;
    build_system(g);
    if (iteration == 0) {                           /* computeLambdaInit (:242-256), tau = 1e-5 */
        double maxDiagonal = 0.;
        for (int j = 0; j < 6; ++j) { const double f = fabs(g->H[7 * j]); maxDiagonal = (f < maxDiagonal) ? maxDiagonal : f; }
        lm->lambda = 1e-5 * maxDiagonal;
        lm->ni = 2;
        lm->nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
        const po_se3 pushed = g->est;               /* _optimizer->push() */
        double Hl[36], x[6] = {0, 0, 0, 0, 0, 0};
        memcpy(Hl, g->H, sizeof(Hl));
        for (int j = 0; j < 6; ++j) Hl[7 * j] += lm->lambda;     /* setLambda(_currentLambda, true) */
        const int ok2 = po_ldlt_solve(Hl, g->b, 6, x);
        po_se3 up;                                   /* update(): VertexSE3Expmap::oplusImpl = exp(update) * estimate */
        po_exp(x, &up);
        po_compose(&up, &g->est, &g->est);
        compute_active_errors(g);
        tempChi = active_robust_chi2(g);
        if (!ok2) tempChi = DBL_MAX;
        rho = (currentChi - tempChi);
        double scale = 0.;                           /* computeScale (:258-267) */
        for (int j = 0; j < 6; ++j) scale += x[j] * (lm->lambda * x[j] + g->b[j]);
        scale += 1e-3;
        rho /= scale;
        if (st) track_min(&st->min_rho, fabs(rho));
        if (rho > 0 && isfinite(tempChi)) {
            double alpha = 1. - pow((2 * rho - 1), 3);
            alpha = (alpha < 2. / 3.) ? alpha : 2. / 3.;              /* std::min(alpha, _goodStepUpperScale) */
            const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;   /* std::max(_goodStepLowerScale, alpha) */
            lm->lambda *= scaleFactor;
            lm->ni = 2;
            currentChi = tempChi;
        } else {
            lm->lambda *= lm->ni;
            lm->ni *= 2;
            g->est = pushed;                         /* pop() */
        }
        qmax++;
    } while (rho < 0 && qmax < 10);
    lm->trials += qmax;
    lm->currentChi = currentChi;
    if (qmax == 10 || rho == 0) return PO_TERMINATE;
    if (st && iniChi != 0) track_min(&st->min_stop, fabs((iniChi - currentChi) * 1e3 - iniChi) / fabs(iniChi));
    if ((iniChi - currentChi) * 1e3 < iniChi) lm->nBad++;     /* Stop criterion (Raul) */
    else lm->nBad = 0;
    if (lm->nBad >= 3) return PO_TERMINATE;
    return PO_OK;
}

/* Optimizer::PoseOptimization (src/Optimizer.cc:264-476).  Frame fields as flat arrays: kp_xy[n][2] = mvKeysUn[i].pt, octave[n],
 * uright[n] = mvuRight (NULL: all -1), has_mp[n] = mvpMapPoints[i] != NULL, mp_pos[n][3] = GetWorldPos, cam = fx fy cx cy mbf,
 * inv_sigma2[nlevels] = mvInvLevelSigma2, Tcw_in = mTcw.  Writes outlier[i] where has_mp[i]; Tcw_out (SetPose) unless fewer
 * than 3 correspondences.  Returns nInitialCorrespondences - nBad.  `edges` = caller scratch of n po_edge. */
int po_pose_optimization(const float *kp_xy, const int32_t *octave, const float *uright, int n, const uint8_t *has_mp, const float *mp_pos,
                         const float cam[5], const float *inv_sigma2, const float Tcw_in[16], float Tcw_out[16], uint8_t *outlier,
                         po_stats *st, po_edge *edges)
{
    po_graph g;
    memset(&g, 0, sizeof(g));
    g.e = edges;
    g.cam.fx = cam[0]; g.cam.fy = cam[1]; g.cam.cx = cam[2]; g.cam.cy = cam[3]; g.cam.bf = cam[4];
    const float deltaMono = sqrt(5.991), deltaStereo = sqrt(7.815);   /* Optimizer.cc:294-295: float */
    g.delta_mono = deltaMono; g.delta_stereo = deltaStereo;
    if (st) { memset(st, 0, sizeof(*st)); st->min_rho = st->min_class = st->min_stop = INFINITY; }
    int nInitial = 0;
    for (int i = 0; i < n; ++i) {
        if (!has_mp[i]) continue;
        po_edge *e = &g.e[g.ne++];
        memset(e, 0, sizeof(*e));
        const float ur = uright ? uright[i] : -1.0f;
        e->stereo = !(ur < 0);
        nInitial++;
        outlier[i] = 0;
        e->obs[0] = kp_xy[2 * i]; e->obs[1] = kp_xy[2 * i + 1]; e->obs[2] = e->stereo ? ur : 0.0;
        const float invSigma2 = inv_sigma2[octave[i]];
        e->info = invSigma2;
        e->robust = 1;
        e->Xw[0] = mp_pos[3 * i]; e->Xw[1] = mp_pos[3 * i + 1]; e->Xw[2] = mp_pos[3 * i + 2];
        e->kp = i;
    }
    if (st) st->ninitial = nInitial;
    if (nInitial < 3) { memcpy(Tcw_out, Tcw_in, 16 * sizeof(float)); return 0; }   /* the pose stays as it was */

    const float chi2Mono[4] = {5.991, 5.991, 5.991, 5.991};
    const float chi2Stereo[4] = {7.815, 7.815, 7.815, 7.815};
    int nBad = 0;
    for (int it = 0; it < 4; it++) {
        po_from_cv(Tcw_in, &g.est);                 /* vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) */
        if (it == 3)
            for (int k = 0; k < g.ne; ++k) g.e[k].level_r4 = g.e[k].level;
        int nactive = 0;
        for (int k = 0; k < g.ne; ++k) nactive += g.e[k].level == 0;
        po_lm lm;
        memset(&lm, 0, sizeof(lm));
        int iters = 0;
        if (nactive > 0) {                          /* else: initializeOptimization finds no active vertex, optimize returns -1 */
            for (int i = 0; i < 10; i++) {          /* SparseOptimizer::optimize (sparse_optimizer.cpp:425-504) */
                const int r = lm_solve(&g, &lm, i, st);
                ++iters;
                if (r != PO_OK) break;
            }
        }
        if (st) {
            st->rounds = it + 1; st->iterations[it] = iters; st->trials[it] = lm.trials;
            st->chi2 = st->round_chi2[it] = iters ? lm.currentChi : 0.0;
            double cp = 0, cr = 0, rho[3];
            for (int k = 0; k < g.ne; ++k) {
                po_edge e = g.e[k];
                if (e.level) continue;
                po_edge_error(&g.cam, e.stereo, e.obs, e.Xw, &g.est, e.err);
                huber(edge_chi2(&e), e.stereo ? g.delta_stereo : g.delta_mono, rho);
                cp += edge_chi2(&e); cr += rho[0];
            }
            st->chi2_plain[it] = cp; st->chi2_robust[it] = cr;
        }
        nBad = 0;
        for (int pass = 0; pass < 2; ++pass)       /* the mono edges first, then the stereo edges (Optimizer.cc:393-448) */
            for (int k = 0; k < g.ne; ++k) {
                po_edge *e = &g.e[k];
                if (e->stereo != pass) continue;
                if (outlier[e->kp]) po_edge_error(&g.cam, e->stereo, e->obs, e->Xw, &g.est, e->err);
                const float chi2 = edge_chi2(e);
                const float th = e->stereo ? chi2Stereo[it] : chi2Mono[it];
                if (st && chi2 == chi2) track_min(&st->min_class, fabs((double)chi2 - th) / th);
                if (chi2 > th) { outlier[e->kp] = 1; e->level = 1; nBad++; }
                else { outlier[e->kp] = 0; e->level = 0; }
                if (it == 2) e->robust = 0;
            }
        if (g.ne < 10) break;                       /* optimizer.edges().size() < 10 */
    }
    po_to_cv(&g.est, Tcw_out);
    if (st) { memcpy(st->q, g.est.q, sizeof(st->q)); memcpy(st->t, g.est.t, sizeof(st->t)); }
    return nInitial - nBad;
}

/* the edge quantities the tests difference numerically: error and chi2 of one edge at T */
double po_edge_chi2(const po_cam *c, int stereo, const double obs[3], const double Xw[3], double info, const po_se3 *T)
{
    po_edge e;
    memset(&e, 0, sizeof(e));
    e.stereo = stereo; e.info = info;
    po_edge_error(c, stereo, obs, Xw, T, e.err);
    return edge_chi2(&e);
}
