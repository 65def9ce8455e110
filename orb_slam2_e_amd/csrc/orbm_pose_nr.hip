// orbm_pose_nr.hip -- Optimizer::PoseOptimizationNR's non-linear optimisation (src/Optimizer.cc:733-809) as ONE launch: one
// workgroup per problem runs the 4 rounds of initializeOptimization(0) + optimize(10), every Levenberg iteration and trial of
// OptimizationAlgorithmLevenberg::solve (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:63-241) with this fork's FEM
// hook (:159-199) inside the kernel, BlockSolver_6_3's Schur step on the one free pose, the inlier / outlier pass between the rounds
// (Optimizer.cc:752-790) and the write-back (:798-809), on the graph the caller has flattened (include/fem_hip.h).  The operation
// order is the restatement's (tests/pose_nr_bundle_oracle.c): EdgeSE3ProjectXYZ (types_six_dof_expmap.h:95-100, .cpp:103-147),
// SE3Quat in quaternion form (orbm_se3.h), Huber with its float dsqr, Eigen's fixed 3 x 3 inverse and pivoting LDLT
// (orbm_g2o_math.h); the hook's arithmetic is fem.hip's own (fem_internal.h), so a trial's sE / nsE are the bits fem_trial_energy
// returns for the same estimates.
//
// Work split: thread t of the 256 owns points t, t + 256, ... and walks its points' edges in edge order (the edges
// arrive grouped by point).  A point's Hll / bl / Hpl therefore sum in edge order in one thread; what joins the threads -- Hpp, bp,
// the robust chi2, the Schur complement, the scale -- is summed per thread and then in a fixed tree (wave butterfly, then the four
// waves in order): no atomics, the same bits from run to run and alone or in a batch.  The 6 x 6 solve, the exp map and every loop
// decision are computed by every lane from the same reduced values, so every barrier is reached by all threads.  The estimates,
// their pushed copy, a and f live in LDS; a point's 30 doubles of Hll, bl, Hpl, an edge's stored error and level and the keyframes'
// poses live in the call's workspace (read and written by the owning thread only, keyframe poses read-only after the prologue).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/fem_hip.h"
#include "../../include/orbslam_hip.h"
#include "common.h"
#include "fem_internal.h"
#include "orbm_g2o_math.h"
#include "orbm_internal.h"
#include "orbm_se3.h"

using namespace orbm_detail;

namespace {

constexpr int NT = 256;                 // threads per problem
constexpr int NW = NT / 64;             // waves
constexpr int NR_MAXTOP = 1365;         // top-layer nodes: Ksize = 6 nTop <= 8,190
constexpr int NR_MAXEDGES = 65536;
constexpr int NR_MAXKF = 1024;
constexpr int NR_MAXOWN = (NR_MAXTOP + NT - 1) / NT;   // points per thread: one bit each in the flag masks
constexpr int NRED = 21 + 6 + 1;        // lower triangle of a 6 x 6, a 6-vector, a scalar
constexpr int NSCHUR = 21 + 6;          // the Schur complement's share of the reduced system
constexpr int SPMV_ROWS = 8;            // rows of K a 16-lane group sums side by side in the hook
static_assert(NR_MAXOWN <= 32, "the per-thread point flags are 32-bit masks");

// One problem as the kernel reads it: device pointers into the model's resident arrays and into the call's workspace.
struct NrProblem {
    // the model (fem_detail::TrialView)
    const float *vals, *u0;
    const int *lcol, *rowptr, *derived, *ids;
    int ndof, nder, nids, sequential;
    float klarge;
    // the graph
    int npoints, nkf, nedges;           // npoints < 0: nothing to do (the host has answered a problem with fewer than 3 points)
    const float *Tcw, *kf_Tcw, *points, *e_obs, *e_info, *e_K;
    const int *e_cam, *e_start;         // e_start[npoints + 1]: a point's edges
    // scratch
    double *blocks;                     // [npoints][30]: Hll (9), bl (3), Hpl (6 x 3)
    double *e_err;                      // [nedges][2]: _error as the last computeError left it
    double *kf_pose;                    // [nkf][7]: q, t
    uint8_t *e_level;                   // [nedges]
    // results
    float *Tout, *points_out;
    uint8_t *outlier;
    int32_t *ngood;
    orbm_pose_nr_stats *stats;          // or nullptr
    orbm_pose_nr_trial *log;            // [log_cap]
    double *points_d;                   // or nullptr
    int log_cap;
};

// EdgeSE3ProjectXYZ::computeError: obs - cam_project(T.map(X)); c = the mapped point
__device__ __forceinline__ void edge_error(const Se3 &T, const double X[3], const float *obs, const float *K, double c[3], double err[2])
{
    se3_map(T, X, c);
    err[0] = (double)obs[0] - (c[0] / c[2] * (double)K[0] + (double)K[2]);
    err[1] = (double)obs[1] - (c[1] / c[2] * (double)K[1] + (double)K[3]);
}

// _error . (information * _error), information = invSigma2 I
__device__ __forceinline__ double edge_chi2(const double err[2], double info) { return err[0] * (info * err[0]) + err[1] * (info * err[1]); }

// linearizeOplus (types_six_dof_expmap.cpp:103-147) at the mapped point c: A = d error / d point (2 x 3), B = d error / d pose (2 x 6)
__device__ __forceinline__ void edge_jacobians(const double c[3], const double R[9], double fx, double fy, double A[6], double B[12])
{
    const double x = c[0], y = c[1], z = c[2], z_2 = z * z;
    const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
    ORBM_UNROLL for (int i = 0; i < 2; ++i)
        ORBM_UNROLL for (int j = 0; j < 3; ++j) A[3 * i + j] = -1. / z * (tmp[3 * i] * R[j] + tmp[3 * i + 1] * R[3 + j] + tmp[3 * i + 2] * R[6 + j]);
    B[0] = x * y / z_2 * fx; B[1] = -(1 + (x * x / z_2)) * fx; B[2] = y / z * fx; B[3] = -1. / z * fx; B[4] = 0; B[5] = x / z_2 * fx;
    B[6] = (1 + y * y / z_2) * fy; B[7] = -x * y / z_2 * fy; B[8] = -x / z * fy; B[9] = 0; B[10] = -1. / z * fy; B[11] = y / z_2 * fy;
}

__device__ __forceinline__ double block_max(double v, double (*red)[NRED])
{
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = v;
    __syncthreads();
    double m = red[0][0];
    ORBM_UNROLL for (int k = 1; k < NW; ++k) m = fmax(m, red[k][0]);
    return m;
}

__global__ __launch_bounds__(NT) void k_pose_nr(const NrProblem *__restrict__ problems)
{
    extern __shared__ __attribute__((aligned(16))) char s_dyn[];
    __shared__ double s_red[NW][NRED];
    __shared__ int s_ired[NW];
    __shared__ double s_sh[NW];

    const NrProblem P = problems[blockIdx.x];
    const int tid = threadIdx.x, np = P.npoints, ndof = P.ndof;
    if (np < 0) return;
    // LDS: the estimates, their pushed copy, a, f (the float top layer is formed in f's first half before f is computed)
    double *sX = reinterpret_cast<double *>(s_dyn), *sXp = sX + 3 * np;
    float *sa = reinterpret_cast<float *>(sXp + 3 * np), *sf = sa + ndof;

    // ---- the graph's vertices: Converter::toSE3Quat of the poses, toVector3d of the points; every edge at level 0
    Se3 est;
    se3_from_cv(P.Tcw, est);
    for (int k = tid; k < P.nkf; k += NT) {
        Se3 T;
        se3_from_cv(P.kf_Tcw + 16 * k, T);
        double *o = P.kf_pose + 7 * k;
        o[0] = T.q[0]; o[1] = T.q[1]; o[2] = T.q[2]; o[3] = T.q[3]; o[4] = T.t[0]; o[5] = T.t[1]; o[6] = T.t[2];
    }
    for (int i = tid; i < 3 * np; i += NT) sX[i] = (double)P.points[i];
    for (int n = tid; n < np; n += NT)
        for (int e = P.e_start[n]; e < P.e_start[n + 1]; ++e) P.e_level[e] = 0;
    __syncthreads();

    auto camera = [&](int cam, Se3 &T) {
        if (cam < 0) { T = est; return; }
        const double *o = P.kf_pose + 7 * cam;
        T.q[0] = o[0]; T.q[1] = o[1]; T.q[2] = o[2]; T.q[3] = o[3]; T.t[0] = o[4]; T.t[1] = o[5]; T.t[2] = o[6];
    };

    const float delta = sqrt(5.991);                    // thHuber, a float in Optimizer.cc
    const float chi2Th = 5.991;                         // chi2[it]
    uint32_t m_out = 0, m_reloc = 0xffffffffu, m_act = 0;   // bit k, the k-th owned point: mvbOutlier, bRelocCheck, active vertex
    int nBad = 0;
    LmStep lm;                                          // OptimizationAlgorithmLevenberg's members
    int nt = 0, nr = 0;
    int st_iter[4] = {0, 0, 0, 0}, st_trials[4] = {0, 0, 0, 0};

    for (int it = 0; it < 4; ++it) {
        // initializeOptimization(0): the level-0 edges and the point vertices they touch
        m_act = 0;
        {
            int k = 0;
            for (int n = tid; n < np; n += NT, ++k)
                for (int e = P.e_start[n]; e < P.e_start[n + 1]; ++e)
                    if (!P.e_level[e]) m_act |= 1u << k;
        }
        for (int iteration = 0; iteration < 10; ++iteration) {                  // SparseOptimizer::optimize
            // ---- computeActiveErrors, activeRobustChi2, buildSystem: v = lower triangle of Hpp, bp, chi2
            double v[NRED];
            for (int j = 0; j < NRED; ++j) v[j] = 0.0;
            double Rest[9];
            quat_to_matrix(est.q, Rest);
            double maxd = 0.;
            {
                int k = 0;
                for (int n = tid; n < np; n += NT, ++k) {
                    if (!((m_act >> k) & 1u)) continue;
                    double H[9], bl[3], Hp[18];
                    for (int j = 0; j < 9; ++j) H[j] = 0.0;
                    for (int j = 0; j < 3; ++j) bl[j] = 0.0;
                    for (int j = 0; j < 18; ++j) Hp[j] = 0.0;
                    const double X[3] = {sX[3 * n], sX[3 * n + 1], sX[3 * n + 2]};
                    for (int e = P.e_start[n]; e < P.e_start[n + 1]; ++e) {
                        if (P.e_level[e]) continue;
                        const int cam = P.e_cam[e];
                        Se3 T;
                        camera(cam, T);
                        const float *K = P.e_K + 4 * e;
                        const double info = (double)P.e_info[e];
                        double c[3], err[2], A[6], B[12], R[9];
                        edge_error(T, X, P.e_obs + 2 * e, K, c, err);
                        P.e_err[2 * e] = err[0]; P.e_err[2 * e + 1] = err[1];
                        double rho0, rho1;
                        huber(edge_chi2(err, info), (double)delta, rho0, rho1);
                        v[27] += rho0;
                        if (cam < 0) { for (int j = 0; j < 9; ++j) R[j] = Rest[j]; }
                        else quat_to_matrix(T.q, R);
                        edge_jacobians(c, R, (double)K[0], (double)K[1], A, B);
                        const double w = rho1 * info;                                   // robustInformation (without rho[2])
                        const double wr0 = -(info * err[0]) * rho1, wr1 = -(info * err[1]) * rho1;
                        ORBM_UNROLL for (int i = 0; i < 3; ++i) {
                            bl[i] += A[i] * wr0 + A[3 + i] * wr1;
                            ORBM_UNROLL for (int j = 0; j < 3; ++j) H[3 * i + j] += A[i] * w * A[j] + A[3 + i] * w * A[3 + j];
                        }
                        if (cam < 0) {
                            ORBM_UNROLL for (int i = 0; i < 6; ++i) {
                                v[21 + i] += B[i] * wr0 + B[6 + i] * wr1;
                                ORBM_UNROLL for (int j = 0; j <= i; ++j) v[i * (i + 1) / 2 + j] += B[i] * w * B[j] + B[6 + i] * w * B[6 + j];
                                ORBM_UNROLL for (int q = 0; q < 3; ++q) Hp[3 * i + q] += B[i] * w * A[q] + B[6 + i] * w * A[3 + q];
                            }
                        }
                    }
                    double *blk = P.blocks + 30 * (size_t)n;
                    for (int j = 0; j < 9; ++j) blk[j] = H[j];
                    for (int j = 0; j < 3; ++j) blk[9 + j] = bl[j];
                    for (int j = 0; j < 18; ++j) blk[12 + j] = Hp[j];
                    for (int j = 0; j < 3; ++j) maxd = fmax(fabs(H[4 * j]), maxd);
                }
            }
            block_sum<NRED, NW>(v, s_red);
            double currentChi = v[27];
            double tempChi = currentChi;
            const double iniChi = currentChi;
            const double *bp = v + 21;                                          // (Hpp stays in v: entry (r, c <= r) at r (r + 1) / 2 + c)
            if (iteration == 0) {                                               // computeLambdaInit over the pose AND the active points, tau = 1e-5
                maxd = block_max(maxd, s_red);
                ORBM_UNROLL for (int j = 0; j < 6; ++j) maxd = fmax(fabs(v[j * (j + 1) / 2 + j]), maxd);
                lm.start(1e-5 * maxd);
            }
            double rho = 0;
            int qmax = 0;
            do {
                // ---- push
                const Se3 pushed = est;
                for (int n = tid; n < np; n += NT) { sXp[3 * n] = sX[3 * n]; sXp[3 * n + 1] = sX[3 * n + 1]; sXp[3 * n + 2] = sX[3 * n + 2]; }
                // ---- setLambda, solve: the Schur complement of the active points on the pose
                double sv[NSCHUR];
                for (int j = 0; j < NSCHUR; ++j) sv[j] = 0.0;
                {
                    int k = 0;
                    for (int n = tid; n < np; n += NT, ++k) {
                        if (!((m_act >> k) & 1u)) continue;
                        const double *blk = P.blocks + 30 * (size_t)n;
                        double D[9], inv[9], W[18];
                        for (int j = 0; j < 9; ++j) D[j] = blk[j];
                        for (int j = 0; j < 3; ++j) D[4 * j] += lm.lambda;
                        inverse3(D, inv);
                        const double *bl = blk + 9, *H = blk + 12;
                        ORBM_UNROLL for (int i = 0; i < 6; ++i)
                            ORBM_UNROLL for (int j = 0; j < 3; ++j) W[3 * i + j] = H[3 * i] * inv[j] + H[3 * i + 1] * inv[3 + j] + H[3 * i + 2] * inv[6 + j];
                        ORBM_UNROLL for (int i = 0; i < 6; ++i) {
                            sv[21 + i] += W[3 * i] * bl[0] + W[3 * i + 1] * bl[1] + W[3 * i + 2] * bl[2];
                            ORBM_UNROLL for (int j = 0; j <= i; ++j) sv[i * (i + 1) / 2 + j] += W[3 * i] * H[3 * j] + W[3 * i + 1] * H[3 * j + 1] + W[3 * i + 2] * H[3 * j + 2];
                        }
                    }
                }
                block_sum<NSCHUR, NW>(sv, s_red);
                double S[36], bs[6], xp[6] = {0, 0, 0, 0, 0, 0};
                for (int j = 0; j < 36; ++j) S[j] = 0.0;                        // (the LDLT reads the lower triangle)
                ORBM_UNROLL for (int r = 0, h = 0; r < 6; ++r)
                    ORBM_UNROLL for (int c = 0; c <= r; ++c, ++h) S[6 * r + c] = (r == c ? v[h] + lm.lambda : v[h]) - sv[h];
                ORBM_UNROLL for (int r = 0; r < 6; ++r) bs[r] = bp[r] - sv[21 + r];
                const bool ok2 = ldlt_solve<6, LdltZeroDiagonal::ReturnZero>(S, bs, xp);
                if (!ok2) for (int j = 0; j < 6; ++j) xp[j] = 0.0;              // x = 0: nothing moves
                // ---- update(x): oplus on the pose and on the active points; computeActiveErrors; the points' share of computeScale
                if (ok2) {
                    Se3 up;
                    se3_exp(xp, up);
                    se3_compose(up, pushed, est);
                }
                double tv[2] = {0.0, 0.0};                                      // robust chi2, scale
                {
                    int k = 0;
                    for (int n = tid; n < np; n += NT, ++k) {
                        if (!((m_act >> k) & 1u)) continue;
                        double X[3] = {sX[3 * n], sX[3 * n + 1], sX[3 * n + 2]};
                        if (ok2) {
                            const double *blk = P.blocks + 30 * (size_t)n;
                            double D[9], inv[9], r[3];
                            for (int j = 0; j < 9; ++j) D[j] = blk[j];
                            for (int j = 0; j < 3; ++j) D[4 * j] += lm.lambda;
                            inverse3(D, inv);
                            const double *bl = blk + 9, *H = blk + 12;
                            ORBM_UNROLL for (int j = 0; j < 3; ++j) {
                                double s = bl[j];
                                ORBM_UNROLL for (int i = 0; i < 6; ++i) s -= H[3 * i + j] * xp[i];
                                r[j] = s;
                            }
                            ORBM_UNROLL for (int j = 0; j < 3; ++j) {
                                const double dx = inv[3 * j] * r[0] + inv[3 * j + 1] * r[1] + inv[3 * j + 2] * r[2];
                                X[j] += dx;
                                tv[1] += dx * (lm.lambda * dx + bl[j]);
                            }
                            sX[3 * n] = X[0]; sX[3 * n + 1] = X[1]; sX[3 * n + 2] = X[2];
                        }
                        for (int e = P.e_start[n]; e < P.e_start[n + 1]; ++e) {
                            if (P.e_level[e]) continue;
                            Se3 T;
                            camera(P.e_cam[e], T);
                            double c[3], err[2];
                            edge_error(T, X, P.e_obs + 2 * e, P.e_K + 4 * e, c, err);
                            P.e_err[2 * e] = err[0]; P.e_err[2 * e + 1] = err[1];
                            double rho0, rho1;
                            huber(edge_chi2(err, (double)P.e_info[e]), (double)delta, rho0, rho1);
                            tv[0] += rho0;
                        }
                    }
                }
                block_sum<2, NW>(tv, s_red);                                    // (its barriers also publish every thread's estimates)
                tempChi = tv[0];
                if (!ok2) tempChi = 1.7976931348623157e308;
                // ---- the hook (:159-199): GetPointCoordinates, Set_uf, ComputeDisplacement, ComputeForces, ComputeStrainEnergy
                float sE, nsE;
                {
                    fem_detail::trial_displacement(sX, np, P.derived, P.nder, P.sequential, sf, P.u0, sa, P.ids, P.nids, P.klarge, tid, NT);
                    __syncthreads();
                    const int sub = tid & 15;
                    for (int r0 = tid >> 4; r0 < ndof; r0 += SPMV_ROWS * (NT / 16)) {    // SPMV_ROWS rows per 16-lane group at a time
                        int k0[SPMV_ROWS], k1[SPMV_ROWS];
                        float s[SPMV_ROWS];
                        ORBM_UNROLL for (int j = 0; j < SPMV_ROWS; ++j) {
                            const int r = r0 + j * (NT / 16);
                            k0[j] = r < ndof ? P.rowptr[r] : 0;
                            k1[j] = r < ndof ? P.rowptr[r + 1] : 0;
                        }
                        fem_detail::fem_row_sum16_rows<SPMV_ROWS>(P.vals, P.lcol, sa, k0, k1, sub, s);
                        ORBM_UNROLL for (int j = 0; j < SPMV_ROWS; ++j) {
                            const int r = r0 + j * (NT / 16);
                            if (sub == 0 && r < ndof) sf[r] = s[j];
                        }
                    }
                    __syncthreads();
                    double s = 0;
                    for (int i = tid; i < ndof; i += NT) s += (double)sa[i] * (double)sf[i];
                    s = fem_detail::block_sum(s, s_sh);
                    fem_detail::strain_energy_of(s, ndof, sE, nsE);
                }
                float w_rE = 1.0, w_sE = 5.0;                                   // :184-185
                if (qmax == 0) {                                                // :186-193
                    w_rE = 1.0;
                    w_sE = 2.0;
                    currentChi += nsE;
                }
                tempChi = w_rE * tempChi + w_sE * nsE;                          // :198 (float * double + float * float)
                double scale = 0.;
                for (int j = 0; j < 6; ++j) scale += xp[j] * (lm.lambda * xp[j] + bp[j]);
                scale += tv[1];
                const LmVerdict vd = lm.verdict(currentChi, tempChi, scale, LmNothing(), [&]() {     // :201-223; an accepted trial: discardTop
                    est = pushed;                                               // pop
                    for (int n = tid; n < np; n += NT) { sX[3 * n] = sXp[3 * n]; sX[3 * n + 1] = sXp[3 * n + 1]; sX[3 * n + 2] = sXp[3 * n + 2]; }
                });
                rho = vd.rho;
                const bool good = vd.accepted;
                if (tid == 0 && nt < P.log_cap) {
                    orbm_pose_nr_trial &t = P.log[nt];
                    t.sE = sE; t.nsE = nsE; t.tempChi = tempChi; t.currentChi = currentChi; t.rho = rho; t.lambda = lm.lambda;
                    t.qmax = qmax; t.accepted = good ? 1 : 0;
                }
                ++nt;
                qmax++;
            } while (rho < 0 && qmax < 10);                                     // :226 (nothing sets terminate() on this path)
            st_iter[it]++;
            st_trials[it] += qmax;
            const int result = lm.end_iteration(qmax, rho, iniChi, currentChi);  // :228-239
            if (tid == 0 && P.stats && nr < 40) P.stats->results[nr] = result;
            ++nr;
            if (result != 1) break;                                             // sparse_optimizer.cpp:470
        }

        // ---- the pass of Optimizer.cc:752-790 in vpEdges order: a point's edges are one thread's, so the flag an earlier edge of the
        // same point has just set is the one the next edge sees
        int bad = 0;
        {
            int k = 0;
            for (int n = tid; n < np; n += NT, ++k) {
                const double X[3] = {sX[3 * n], sX[3 * n + 1], sX[3 * n + 2]};
                for (int e = P.e_start[n]; e < P.e_start[n + 1]; ++e) {
                    double err[2] = {P.e_err[2 * e], P.e_err[2 * e + 1]};
                    if ((m_out >> k) & 1u) {                                    // e->computeError()
                        Se3 T;
                        camera(P.e_cam[e], T);
                        double c[3];
                        edge_error(T, X, P.e_obs + 2 * e, P.e_K + 4 * e, c, err);
                        P.e_err[2 * e] = err[0]; P.e_err[2 * e + 1] = err[1];
                    }
                    const double chi2 = edge_chi2(err, (double)P.e_info[e]);
                    if (chi2 > chi2Th) {
                        m_out |= 1u << k;
                        P.e_level[e] = 1;
                        if ((m_reloc >> k) & 1u) { bad++; m_reloc &= ~(1u << k); }
                    } else if (chi2 <= chi2Th) {                                // (a NaN falls through both, as there)
                        m_out &= ~(1u << k);
                        P.e_level[e] = 0;
                        if (!((m_reloc >> k) & 1u)) { m_reloc |= 1u << k; bad--; }
                    }
                }
            }
        }
        nBad = block_sum_int<NW>(bad, s_ired);                                  // nBad = 0 at :752: the last round's only
    }

    // ---- :798-809: Converter::toCvMat of the pose and of the points
    {
        int k = 0;
        for (int n = tid; n < np; n += NT, ++k) {
            P.outlier[n] = (m_out >> k) & 1u;
            for (int j = 0; j < 3; ++j) {
                P.points_out[3 * n + j] = (float)sX[3 * n + j];
                if (P.points_d) P.points_d[3 * n + j] = sX[3 * n + j];
            }
        }
    }
    if (tid == 0) {
        double R[9];
        quat_to_matrix(est.q, R);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) P.Tout[4 * i + j] = (float)R[3 * i + j];
            P.Tout[4 * i + 3] = (float)est.t[i];
        }
        P.Tout[12] = 0.f; P.Tout[13] = 0.f; P.Tout[14] = 0.f; P.Tout[15] = 1.f;
        *P.ngood = np - nBad;
        if (P.stats) {
            orbm_pose_nr_stats &s = *P.stats;
            s.rounds = 4;
            for (int j = 0; j < 4; ++j) { s.iterations[j] = st_iter[j]; s.trials[j] = st_trials[j]; }
            s.nresults = nr;
            for (int j = nr; j < 40; ++j) s.results[j] = 0;
            s.trial_capacity = P.log_cap; s.ntrials = nt; s.trial_overflow = nt > P.log_cap ? 1 : 0; s.reserved = 0;
            s.trial_log = nullptr; s.points = nullptr;                          // the caller's pointers stay the caller's
            for (int j = 0; j < 4; ++j) s.q[j] = est.q[j];
            for (int j = 0; j < 3; ++j) s.t[j] = est.t[j];
        }
    }
}

// ---- host

size_t lds_bytes(int npoints, int ndof) { return sizeof(double) * 6 * (size_t)npoints + sizeof(float) * 2 * (size_t)ndof; }

// the graph alone (no model, no device): limits, indices, grouping; fills e_start[npoints + 1]
int check_graph(const orbm_pose_nr_graph &g, std::vector<int32_t> &e_start)
{
    if (g.npoints < 0 || g.nkf < 0 || g.nedges < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative size");
    if (!g.Tcw || (g.nkf && !g.kf_Tcw) || (g.npoints && !g.points) ||
        (g.nedges && (!g.e_point || !g.e_cam || !g.e_obs || !g.e_inv_sigma2 || !g.e_cam_k)))
        ORBX_FAIL(ORBX_ERR_ARG, "null pointer in the graph");
    if (g.npoints > NR_MAXTOP) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,365 top-layer nodes (Ksize > 8,190): use PoseOptimizationNR_fem");
    if (g.nedges > NR_MAXEDGES) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 65,536 edges");
    if (g.nkf > NR_MAXKF) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,024 keyframes");
    e_start.assign((size_t)g.npoints + 1, 0);
    int prev = 0;
    for (int e = 0; e < g.nedges; ++e) {
        const int p = g.e_point[e], c = g.e_cam[e];
        if (p < 0 || p >= g.npoints) ORBX_FAIL(ORBX_ERR_ARG, "an edge's point index is out of range");
        if (c < -1 || c >= g.nkf) ORBX_FAIL(ORBX_ERR_ARG, "an edge's camera index is out of range");
        if (p < prev) ORBX_FAIL(ORBX_ERR_ARG, "edges must be grouped by point, points ascending");
        prev = p;
        e_start[(size_t)p + 1]++;
    }
    for (int n = 0; n < g.npoints; ++n) e_start[(size_t)n + 1] += e_start[n];
    return ORBX_OK;
}

// Optimizer.cc:711-714: fewer than 3 correspondences
void answer_degenerate(const orbm_pose_nr_graph &g, orbm_pose_nr_result &out, orbm_pose_nr_stats *st)
{
    memcpy(out.Tcw, g.Tcw, sizeof(float) * 16);
    for (int i = 0; i < 3 * g.npoints; ++i) out.points_out[i] = g.points[i];
    for (int i = 0; i < g.npoints; ++i) out.outlier[i] = 0;
    out.ngood = 0;
    if (st) {
        orbm_pose_nr_trial *log = st->trial_log;
        double *pts = st->points;
        const int cap = st->trial_capacity;
        memset(st, 0, sizeof(*st));
        st->trial_log = log; st->points = pts; st->trial_capacity = cap;
        for (int i = 0; pts && i < 3 * g.npoints; ++i) pts[i] = g.points[i];
    }
}

int pose_nr_run(fem_model *const *models, const orbm_pose_nr_graph *graphs, int batch, orbm_pose_nr_result *out, orbm_pose_nr_stats *stats,
                bool on_model_stream)
{
    if (!graphs || !out || (batch > 0 && !models)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    std::vector<std::vector<int32_t>> e_start((size_t)batch);
    std::vector<fem_detail::TrialView> view((size_t)batch);
    int live = 0;
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        const int rc = check_graph(g, e_start[b]);
        if (rc != ORBX_OK) return rc;
        if (g.npoints && (!out[b].points_out || !out[b].outlier)) ORBX_FAIL(ORBX_ERR_ARG, "null result array");
        if (stats && stats[b].trial_capacity < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative trial capacity");
        if (stats && stats[b].trial_capacity > 0 && !stats[b].trial_log) ORBX_FAIL(ORBX_ERR_ARG, "trial capacity without a trial log");
    }
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        if (g.npoints < 3) continue;
        if (!fem_detail::trial_view(models[b], &view[b])) ORBX_FAIL(ORBX_ERR_ARG, "the model must be one mesh (fem_create) with fem_trial_setup done");
        if (view[b].npoints != g.npoints) ORBX_FAIL(ORBX_ERR_ARG, "fem_trial_setup was made for another number of points");
        if (view[b].ndof > 6 * NR_MAXTOP) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,365 top-layer nodes (Ksize > 8,190): use PoseOptimizationNR_fem");
        ++live;
    }
    if (!live) {
        for (int b = 0; b < batch; ++b) answer_degenerate(graphs[b], out[b], stats ? stats + b : nullptr);
        return ORBX_OK;
    }
    ORBX_NEED_DEVICE();

    StagedCall sc;
    std::vector<NrProblem> probs((size_t)batch);
    struct Off { size_t tcw, kf, pts, obs, info, K, cam, es, blocks, err, kfp, lvl, tout, pout, outl, ngood, stats, log, ptsd; };
    std::vector<Off> off((size_t)batch);
    const size_t o_probs = sc.in(nullptr, sizeof(NrProblem) * (size_t)batch);
    size_t lds = 0;
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        Off &o = off[b];
        if (g.npoints < 3) continue;
        const size_t np = (size_t)g.npoints, ne = (size_t)g.nedges, nk = (size_t)g.nkf;
        o.tcw = sc.in(g.Tcw, sizeof(float) * 16); o.kf = sc.in(g.kf_Tcw, sizeof(float) * 16 * nk); o.pts = sc.in(g.points, sizeof(float) * 3 * np);
        o.obs = sc.in(g.e_obs, sizeof(float) * 2 * ne); o.info = sc.in(g.e_inv_sigma2, sizeof(float) * ne); o.K = sc.in(g.e_cam_k, sizeof(float) * 4 * ne);
        o.cam = sc.in(g.e_cam, sizeof(int32_t) * ne); o.es = sc.in(e_start[b].data(), sizeof(int32_t) * (np + 1));
        lds = std::max(lds, lds_bytes(g.npoints, view[b].ndof));
    }
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        Off &o = off[b];
        if (g.npoints < 3) continue;
        o.blocks = sc.scratch(sizeof(double) * 30 * (size_t)g.npoints); o.err = sc.scratch(sizeof(double) * 2 * (size_t)g.nedges);
        o.kfp = sc.scratch(sizeof(double) * 7 * (size_t)g.nkf); o.lvl = sc.scratch((size_t)g.nedges);
    }
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        Off &o = off[b];
        if (g.npoints < 3) continue;
        const size_t np = (size_t)g.npoints;
        o.tout = sc.out(sizeof(float) * 16); o.pout = sc.out(sizeof(float) * 3 * np); o.outl = sc.out(np); o.ngood = sc.out(sizeof(int32_t));
        o.stats = sc.out(sizeof(orbm_pose_nr_stats));
        o.log = sc.out(sizeof(orbm_pose_nr_trial) * (size_t)(stats ? stats[b].trial_capacity : 0));
        o.ptsd = sc.out(sizeof(double) * 3 * (stats && stats[b].points ? np : 0));
    }
    // the problem table holds device addresses: the arena must have its final size before they are formed
    if (on_model_stream) {
        for (int b = 0; b < batch; ++b)
            if (graphs[b].npoints >= 3) sc.on = view[b].stream;
    }
    {
        const size_t need = sc.w.used;
        const char *before = sc.w.dev;
        if (sc.w.reserve(need, std::max(sc.staged, sc.res_bytes))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
        sc.w.used = need;
        if (sc.w.dev != before) ORBX_HIP(hipStreamSynchronize(sc.w.st));      // a grown arena is zeroed on the workspace's stream
    }
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        NrProblem &p = probs[b];
        memset(&p, 0, sizeof(p));
        p.npoints = -1;
        if (g.npoints < 3) continue;
        const fem_detail::TrialView &v = view[b];
        const Off &o = off[b];
        p.vals = v.vals; p.u0 = v.u0; p.lcol = v.lcol; p.rowptr = v.rowptr; p.derived = v.derived; p.ids = v.ids;
        p.ndof = v.ndof; p.nder = v.nder; p.nids = v.nids; p.sequential = v.sequential; p.klarge = v.klarge;
        p.npoints = g.npoints; p.nkf = g.nkf; p.nedges = g.nedges;
        p.Tcw = sc.d<float>(o.tcw); p.kf_Tcw = sc.d<float>(o.kf); p.points = sc.d<float>(o.pts); p.e_obs = sc.d<float>(o.obs);
        p.e_info = sc.d<float>(o.info); p.e_K = sc.d<float>(o.K); p.e_cam = sc.d<int>(o.cam); p.e_start = sc.d<int>(o.es);
        p.blocks = sc.d<double>(o.blocks); p.e_err = sc.d<double>(o.err); p.kf_pose = sc.d<double>(o.kfp); p.e_level = sc.d<uint8_t>(o.lvl);
        p.Tout = sc.d<float>(o.tout); p.points_out = sc.d<float>(o.pout); p.outlier = sc.d<uint8_t>(o.outl); p.ngood = sc.d<int32_t>(o.ngood);
        p.stats = stats ? sc.d<orbm_pose_nr_stats>(o.stats) : nullptr;
        p.log = sc.d<orbm_pose_nr_trial>(o.log); p.log_cap = stats ? stats[b].trial_capacity : 0;
        p.points_d = stats && stats[b].points ? sc.d<double>(o.ptsd) : nullptr;
    }
    sc.in_at(o_probs, probs.data(), sizeof(NrProblem) * (size_t)batch);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    static const hipError_t lds_attr = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pose_nr), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                            (int)lds_bytes(NR_MAXTOP, 6 * NR_MAXTOP));   // once: the largest problem's LDS
    ORBX_HIP(lds_attr);
    hipLaunchKernelGGL(k_pose_nr, dim3(batch), dim3(NT), lds, sc.stream(), sc.d<NrProblem>(o_probs));
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    for (int b = 0; b < batch; ++b) {
        const orbm_pose_nr_graph &g = graphs[b];
        if (g.npoints < 3) { answer_degenerate(g, out[b], stats ? stats + b : nullptr); continue; }
        const Off &o = off[b];
        const size_t np = (size_t)g.npoints;
        memcpy(out[b].Tcw, sc.r<float>(o.tout), sizeof(float) * 16);
        memcpy(out[b].points_out, sc.r<float>(o.pout), sizeof(float) * 3 * np);
        memcpy(out[b].outlier, sc.r<uint8_t>(o.outl), np);
        out[b].ngood = *sc.r<int32_t>(o.ngood);
        if (stats) {
            orbm_pose_nr_stats &s = stats[b];
            orbm_pose_nr_trial *log = s.trial_log;
            double *pts = s.points;
            s = *sc.r<orbm_pose_nr_stats>(o.stats);
            s.trial_log = log; s.points = pts;
            const int nlog = s.ntrials < s.trial_capacity ? s.ntrials : s.trial_capacity;
            if (nlog > 0) memcpy(log, sc.r<orbm_pose_nr_trial>(o.log), sizeof(orbm_pose_nr_trial) * (size_t)nlog);
            if (pts) memcpy(pts, sc.r<double>(o.ptsd), sizeof(double) * 3 * np);
        }
    }
    return ORBX_OK;
}

} // namespace

int orbm_pose_optimization_nr(fem_model *m, const orbm_pose_nr_graph *g, orbm_pose_nr_result *out, orbm_pose_nr_stats *stats)
{
    fem_model *const models[1] = {m};
    return pose_nr_run(models, g, 1, out, stats, true);
}

int orbm_pose_optimization_nr_batch(fem_model *const *models, const orbm_pose_nr_graph *graphs, int batch, orbm_pose_nr_result *out,
                                    orbm_pose_nr_stats *stats)
{
    if (batch < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative batch");
    if (batch == 0) return ORBX_OK;
    return pose_nr_run(models, graphs, batch, out, stats, false);
}
