// orbm_ba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:837-1162) and Optimizer::BundleAdjustment (:74-262) on the graph
// the caller has flattened (include/orbslam_hip.h).  The DECISIONS stay on the host: OptimizationAlgorithmLevenberg::solve
// (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:63-241, bInFEA false) with its trial loop, lambda and _ni, rho with
// + 1e-3, qmax, _nBad and Terminate, SparseOptimizer::optimize's loop (sparse_optimizer.cpp:453) and the stop flag where g2o reads
// it.  The PASSES run on the device, each over the whole chip, and no workgroup ever waits for another:
//   k_ba_errors       computeError of every active edge (EdgeSE3ProjectXYZ types_six_dof_expmap.h:95-100, EdgeStereoSE3ProjectXYZ
//                     with cam_project's float invz, .cpp:150-157), stored per edge; the robust chi2 per thread, wave, block
//   k_ba_build        linearizeOplus (.cpp:103-139, :188-234) + constructQuadraticForm with robustInformation as orbm_pose_nr.hip
//                     applies it: a point's Hll / bl summed over its edges in edge order by ONE thread, an edge's 6 x 3 Hpl block and
//                     its 27 contributions to Hpp / bp
//   k_ba_pose         a free pose's Hpp / bp: lane j sums contribution j over the pose's edge list, in edge order
//   k_ba_dinv         Dinv = (Hll + lambda I)^-1 (Eigen's fixed 3 x 3 inverse) and Dinv bl per active point
//   k_ba_schur        BlockSolver::solve (core/block_solver.hpp:354-496): one wave per upper block (i1 <= i2), lane (r, c) subtracts
//                     (B_i1 Dinv) B_i2^T entry by entry over the block's (point, edge, edge) list, points ascending; bschur likewise
//   k_ba_solve        dense LLT of the 6 nact reduced system, lower triangle, every entry's dot product in ascending k; ONE
//                     workgroup; the matrix lives in the workspace, a row at a time goes through LDS.  orbm_global_bundle_adjustment
//                     (up to 512 free keyframes, a system up to 3,072 wide) calls orbm_llt_solve_dev (orbm_llt.hip) in its place:
//                     the same operations in the same order over many workgroups, hence the same bytes
//   k_ba_schur_env    orbm_global_bundle_adjustment_env (up to 4,096 free keyframes): the same entries, a wave per
//                     block of the COMPACT list of non-empty blocks, into the live tiles of the system's tile envelope, which a fill
//                     on the stream has set to +0.0; orbm_llt_env_solve_dev solves there.  The square S does not exist on that path
//   k_ba_update(_pose) push; xl = Dinv (bl - B^T xp); oplus on points and poses; computeScale's terms
//   k_ba_reduce       the block partials of chi2 / scale / the largest diagonal entry joined in a fixed tree
//   k_ba_pop, k_ba_classify, k_ba_activate, k_ba_final   the copies, the level pass, initializeOptimization(0)'s vertex set, write-back
// Sums that join threads: per thread in index order, wave butterfly, then the block partials per thread in index order and the
// butterfly / wave order again.  No floating-point atomics: a call gives the same bytes from run to run.  The host waits once per
// trial (a 128-byte block: tempChi, scale, ok2) and once per round.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../../include/orbslam_hip.h"
#include "common.h"
#include "orbm_g2o_math.h"
#include "orbm_internal.h"
#include "orbm_llt_env.h"
#include "orbm_se3.h"

using namespace orbm_detail;

namespace {

constexpr int PT = 64;                  // threads per block of the per-point / per-edge passes: one wave
constexpr int RT = 256;                 // the reduction's one block
constexpr int ST = 384;                 // the solve's one block: a thread per row of the largest system
constexpr int BA_MAXFREE = 64, BA_MAXFIXED = 1024, BA_MAXPOINTS = 65536, BA_MAXEDGES = 524288, BA_MAXITER = 64;
static_assert(ST == 6 * BA_MAXFREE, "a thread per row");
// orbm_global_bundle_adjustment: the tiled solve takes the reduced system of 512 keyframes; its block-entry list is capped (403 MB)
constexpr int BA_MAXFREE_GLOBAL = 512;
constexpr int64_t BA_MAXBLOCKENT_GLOBAL = (int64_t)1 << 25;
static_assert(BA_MAXFREE_GLOBAL * (BA_MAXFREE_GLOBAL + 1) / 2 < (1 << 30), "block indices are ints");
// orbm_global_bundle_adjustment_env: the envelope solve takes 28,672 rows; the block list holds the non-empty blocks only (805 MB at its cap)
constexpr int BA_MAXFREE_ENV = 4096, BA_MAXPOINTS_ENV = 1 << 20, BA_MAXEDGES_ENV = 1 << 22;
constexpr int64_t BA_MAXBLOCKENT_ENV = (int64_t)1 << 26;
constexpr int BA_ENV_MAXTILES = 8192;   // orbm_llt_env_solve_dev's cap on live tiles
static_assert(6 * BA_MAXFREE_ENV <= 28672, "the system fits orbm_llt_env_solve_dev");
static_assert(BA_MAXBLOCKENT_ENV < 0x7fffffff, "block_start holds ints (3 k, the index into the entries, is formed as size_t)");
enum { BA_LOCAL = 0, BA_GLOBAL = 1, BA_ENV = 2 };      // the three public entries of the one body

// the call's arrays on the device
struct BaDev {
    int nfree, npose, npoints, nedges, nblocks;     // nblocks: blocks of the per-point passes
    const float *poses_in, *points_in, *e_obs, *e_info, *e_K;
    const int *e_cam, *e_start, *pose_class, *pe_start, *pe_list, *blk_start, *blk_ent;
    const int *blk_i1, *blk_i2;         // [listed blocks]: the env entry's compact list, sorted by (i1, i2)
    const int *env;                     // the envelope's device plan image (orbm_llt_env.h)
    double *A, *W;                      // the live tiles and the solver's running dots
    int T, nt;                          // tile edge; row tiles of the round's system
    double *est, *est_bak;              // [npose][7], [nfree][7]: q, t
    double *X, *X_bak;                  // [npoints][3]
    double *e_err;                      // [nedges][3]: _error as the last computeError that had the edge active left it
    double *Hll;                        // [npoints][12]: Hll, bl
    double *Dinv;                       // [npoints][12]: (Hll + lambda I)^-1, Dinv bl
    double *Hpl;                        // [nedges][18]
    double *contrib;                    // [nedges][27]: the edge's share of Hpp (lower triangle) and bp
    double *Hpp;                        // [nfree][27]
    double *pose_max, *pose_scale;      // [nfree]
    double *S, *bsch, *xp;              // the reduced system, column-major lower triangle [n][n], [n], [n]
    double *part_chi, *part_max, *part_scale;   // [nblocks]
    uint8_t *e_level, *pact;            // [nedges], [npoints]
    int *ridx;                          // [nfree]: row block in the reduced system, -1: not a vertex of this round
    double *sc;                         // the block a trial reads back (LM_SC_*, LM_ISC_*: orbm_internal.h)
    int *isc;
    float *poses_out, *points_out;
    uint8_t *erase, *level_out;
    double *chi2_out, *poses_d, *points_d;
};

__device__ __forceinline__ void load_pose(const double *est, int k, Se3 &T)
{
    const double *o = est + 7 * (size_t)k;
    T.q[0] = o[0]; T.q[1] = o[1]; T.q[2] = o[2]; T.q[3] = o[3]; T.t[0] = o[4]; T.t[1] = o[5]; T.t[2] = o[6];
}
__device__ __forceinline__ void store_pose(double *est, int k, const Se3 &T)
{
    double *o = est + 7 * (size_t)k;
    o[0] = T.q[0]; o[1] = T.q[1]; o[2] = T.q[2]; o[3] = T.q[3]; o[4] = T.t[0]; o[5] = T.t[1]; o[6] = T.t[2];
}

// computeError of either edge type at the mapped point c; a monocular edge (obs[2] < 0) has err[2] = 0
__device__ __forceinline__ void ba_error(const double c[3], const float *obs, const float *K, double err[3])
{
    const double fx = (double)K[0], fy = (double)K[1], cx = (double)K[2], cy = (double)K[3];
    if (obs[2] < 0.f) {
        err[0] = (double)obs[0] - (c[0] / c[2] * fx + cx);
        err[1] = (double)obs[1] - (c[1] / c[2] * fy + cy);
        err[2] = 0.0;
    } else {
        const float invz = (float)(1.0 / c[2]);                 // const float invz = 1.0f / trans_xyz[2]
        const double r0 = c[0] * (double)invz * fx + cx;
        const double r1 = c[1] * (double)invz * fy + cy;
        const double r2 = r0 - (double)(K[4] * invz);           // bf * invz: a float product
        err[0] = (double)obs[0] - r0; err[1] = (double)obs[1] - r1; err[2] = (double)obs[2] - r2;
    }
}

// chi2(): _error . (information * _error), information = invSigma2 I (the third term of a monocular edge is + 0)
__device__ __forceinline__ double ba_chi2(const double err[3], double info) { return err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]); }

// linearizeOplus of either edge type: A = d error / d point (3 x 3), B = d error / d pose (3 x 6); a monocular edge's third rows are 0
__device__ __forceinline__ void ba_jacobians(const double c[3], const double R[9], const float *K, bool stereo, double A[9], double B[18])
{
    const double fx = (double)K[0], fy = (double)K[1], bf = (double)K[4];
    const double x = c[0], y = c[1], z = c[2], z_2 = z * z;
    if (!stereo) {
        const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
        ORBM_UNROLL for (int i = 0; i < 2; ++i)
            ORBM_UNROLL for (int j = 0; j < 3; ++j) A[3 * i + j] = -1. / z * (tmp[3 * i] * R[j] + tmp[3 * i + 1] * R[3 + j] + tmp[3 * i + 2] * R[6 + j]);
        A[6] = 0; A[7] = 0; A[8] = 0;
    } else {
        ORBM_UNROLL for (int j = 0; j < 3; ++j) {
            A[j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
            A[3 + j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
            A[6 + j] = A[j] - bf * R[6 + j] / z_2;
        }
    }
    B[0] = x * y / z_2 * fx; B[1] = -(1 + (x * x / z_2)) * fx; B[2] = y / z * fx; B[3] = -1. / z * fx; B[4] = 0; B[5] = x / z_2 * fx;
    B[6] = (1 + y * y / z_2) * fy; B[7] = -x * y / z_2 * fy; B[8] = -x / z * fy; B[9] = 0; B[10] = -1. / z * fy; B[11] = y / z_2 * fy;
    if (stereo) {
        B[12] = B[0] - bf * y / z_2; B[13] = B[1] + bf * x / z_2; B[14] = B[2]; B[15] = B[3]; B[16] = 0; B[17] = B[5] - bf / z_2;
    } else {
        ORBM_UNROLL for (int j = 12; j < 18; ++j) B[j] = 0;
    }
}

// Converter::toSE3Quat / toVector3d; every edge at level 0
__global__ __launch_bounds__(PT) void k_ba_init(BaDev D)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < D.npose) {
        Se3 T;
        se3_from_cv(D.poses_in + 16 * (size_t)i, T);
        store_pose(D.est, i, T);
        if (i < D.nfree) store_pose(D.est_bak, i, T);
    }
    if (i < D.npoints)
        for (int j = 0; j < 3; ++j) { D.X[3 * (size_t)i + j] = (double)D.points_in[3 * (size_t)i + j]; D.X_bak[3 * (size_t)i + j] = D.X[3 * (size_t)i + j]; }
    if (i < D.nedges) {
        D.e_level[i] = 0;
        for (int j = 0; j < 3; ++j) D.e_err[3 * (size_t)i + j] = 0.0;
    }
}

// initializeOptimization(level 0): a vertex is in the system iff one of its edges is on level 0.  One block.
__global__ __launch_bounds__(RT) void k_ba_activate(BaDev D)
{
    __shared__ int s_act[BA_MAXFREE_ENV];
    __shared__ int s_edges;
    if (threadIdx.x == 0) s_edges = 0;
    __syncthreads();
    int mine = 0;
    for (int n = threadIdx.x; n < D.npoints; n += RT) {
        int a = 0;
        for (int e = D.e_start[n]; e < D.e_start[n + 1]; ++e) a += D.e_level[e] == 0;
        D.pact[n] = a > 0;
        mine += a;
    }
    atomicAdd(&s_edges, mine);                                  // (an integer count)
    for (int p = threadIdx.x; p < D.nfree; p += RT) {
        int a = 0;
        if (D.pose_class[p] == 0)
            for (int k = D.pe_start[p]; k < D.pe_start[p + 1] && !a; ++k) a = D.e_level[D.pe_list[k]] == 0;
        s_act[p] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int p = 0; p < D.nfree; ++p) D.ridx[p] = s_act[p] ? r++ : -1;
        D.isc[LM_ISC_NACT] = r; D.isc[LM_ISC_OK2] = 1; D.isc[LM_ISC_NEDGES] = s_edges;
    }
}

// computeActiveErrors + activeRobustChi2
__global__ __launch_bounds__(PT) void k_ba_errors(BaDev D, int robust, double dm, double ds)
{
    const int n = blockIdx.x * PT + threadIdx.x;
    double chi = 0.0;
    if (n < D.npoints && D.pact[n]) {
        const double X[3] = {D.X[3 * (size_t)n], D.X[3 * (size_t)n + 1], D.X[3 * (size_t)n + 2]};
        for (int e = D.e_start[n]; e < D.e_start[n + 1]; ++e) {
            if (D.e_level[e]) continue;
            Se3 T;
            load_pose(D.est, D.e_cam[e], T);
            double c[3], err[3];
            se3_map(T, X, c);
            const float *obs = D.e_obs + 3 * (size_t)e;
            ba_error(c, obs, D.e_K + 5 * (size_t)e, err);
            D.e_err[3 * (size_t)e] = err[0]; D.e_err[3 * (size_t)e + 1] = err[1]; D.e_err[3 * (size_t)e + 2] = err[2];
            const double c2 = ba_chi2(err, (double)D.e_info[e]);
            if (robust) {
                double rho0, rho1;
                huber(c2, obs[2] < 0.f ? dm : ds, rho0, rho1);
                chi += rho0;
            } else
                chi += c2;
        }
    }
    chi = wave_sum(chi);
    if (threadIdx.x == 0) D.part_chi[blockIdx.x] = chi;
}

// buildSystem: the Jacobians at the current estimates, the stored error, robustInformation without rho[2]
__global__ __launch_bounds__(PT) void k_ba_build(BaDev D, int robust, double dm, double ds)
{
    const int n = blockIdx.x * PT + threadIdx.x;
    double maxd = 0.0;
    if (n < D.npoints && D.pact[n]) {
        double H[9], bl[3];
        ORBM_UNROLL for (int j = 0; j < 9; ++j) H[j] = 0.0;
        ORBM_UNROLL for (int j = 0; j < 3; ++j) bl[j] = 0.0;
        const double X[3] = {D.X[3 * (size_t)n], D.X[3 * (size_t)n + 1], D.X[3 * (size_t)n + 2]};
        for (int e = D.e_start[n]; e < D.e_start[n + 1]; ++e) {
            if (D.e_level[e]) continue;
            const int cam = D.e_cam[e];
            Se3 T;
            load_pose(D.est, cam, T);
            double c[3], R[9], A[9], B[18];
            se3_map(T, X, c);
            quat_to_matrix(T.q, R);
            const float *obs = D.e_obs + 3 * (size_t)e;
            const bool stereo = !(obs[2] < 0.f);
            ba_jacobians(c, R, D.e_K + 5 * (size_t)e, stereo, A, B);
            const double err[3] = {D.e_err[3 * (size_t)e], D.e_err[3 * (size_t)e + 1], D.e_err[3 * (size_t)e + 2]};
            const double info = (double)D.e_info[e];
            double rho0 = 0, rho1 = 1.;
            if (robust) huber(ba_chi2(err, info), stereo ? ds : dm, rho0, rho1);
            const double w = rho1 * info;
            const double wr0 = -(info * err[0]) * rho1, wr1 = -(info * err[1]) * rho1, wr2 = -(info * err[2]) * rho1;
            ORBM_UNROLL for (int i = 0; i < 3; ++i) {
                bl[i] += A[i] * wr0 + A[3 + i] * wr1 + A[6 + i] * wr2;
                ORBM_UNROLL for (int j = 0; j < 3; ++j) H[3 * i + j] += A[i] * w * A[j] + A[3 + i] * w * A[3 + j] + A[6 + i] * w * A[6 + j];
            }
            if (cam < D.nfree && D.ridx[cam] >= 0) {
                double *hp = D.Hpl + 18 * (size_t)e, *cb = D.contrib + 27 * (size_t)e;
                ORBM_UNROLL for (int i = 0; i < 6; ++i) {
                    cb[21 + i] = B[i] * wr0 + B[6 + i] * wr1 + B[12 + i] * wr2;
                    ORBM_UNROLL for (int j = 0; j <= i; ++j) cb[i * (i + 1) / 2 + j] = B[i] * w * B[j] + B[6 + i] * w * B[6 + j] + B[12 + i] * w * B[12 + j];
                    ORBM_UNROLL for (int q = 0; q < 3; ++q) hp[3 * i + q] = B[i] * w * A[q] + B[6 + i] * w * A[3 + q] + B[12 + i] * w * A[6 + q];
                }
            }
        }
        double *blk = D.Hll + 12 * (size_t)n;
        ORBM_UNROLL for (int j = 0; j < 9; ++j) blk[j] = H[j];
        ORBM_UNROLL for (int j = 0; j < 3; ++j) blk[9 + j] = bl[j];
        ORBM_UNROLL for (int j = 0; j < 3; ++j) maxd = fmax(fabs(H[4 * j]), maxd);
    }
    maxd = wave_max(maxd);
    if (threadIdx.x == 0) D.part_max[blockIdx.x] = maxd;
}

// Hpp / bp of free pose blockIdx.x: lane j sums contribution j over the pose's edges in edge order
__global__ __launch_bounds__(PT) void k_ba_pose(BaDev D)
{
    const int p = blockIdx.x, j = threadIdx.x;
    double s = 0.0;
    const bool act = D.ridx[p] >= 0;
    if (act && j < 27)
        for (int k = D.pe_start[p]; k < D.pe_start[p + 1]; ++k) {
            const int e = D.pe_list[k];
            if (D.e_level[e]) continue;
            s += D.contrib[27 * (size_t)e + j];
        }
    if (j < 27) D.Hpp[27 * p + j] = s;
    const bool diag = j == 0 || j == 2 || j == 5 || j == 9 || j == 14 || j == 20;
    const double m = wave_max(diag && act ? fabs(s) : 0.0);
    if (j == 0) D.pose_max[p] = m;
}

// mode 0: chi2 at the iteration's start, computeLambdaInit's largest diagonal entry and tau times it.  mode 1: tempChi and
// computeScale: the poses' terms in pose order by one thread, the points' block partials in the tree.  One block.
__global__ __launch_bounds__(RT) void k_ba_reduce(BaDev D, int mode)
{
    __shared__ double s_red[RT / 64][2];
    double v[2] = {0.0, 0.0}, mx = 0.0;
    for (int b = threadIdx.x; b < D.nblocks; b += RT) {
        v[0] += D.part_chi[b];
        if (mode) v[1] += D.part_scale[b];
        else mx = fmax(mx, D.part_max[b]);
    }
    if (!mode)
        for (int p = threadIdx.x; p < D.nfree; p += RT) mx = fmax(mx, D.pose_max[p]);
    block_sum<2, RT / 64>(v, s_red);
    if (!mode) {
        mx = wave_max(mx);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][0] = mx;
        __syncthreads();
        mx = fmax(fmax(s_red[0][0], s_red[1][0]), fmax(s_red[2][0], s_red[3][0]));
    }
    if (threadIdx.x == 0) {
        if (!mode) { D.sc[LM_SC_CHI2] = v[0]; D.sc[LM_SC_MAXDIAG] = mx; D.sc[LM_SC_LAMBDA_INIT] = 1e-5 * mx; }
        else {
            double sp = 0.0;
            for (int p = 0; p < D.nfree; ++p) sp += D.pose_scale[p];
            D.sc[LM_SC_TEMPCHI] = v[0]; D.sc[LM_SC_SCALE] = sp + v[1];
        }
    }
}

__global__ __launch_bounds__(PT) void k_ba_dinv(BaDev D, double lambda, int lambda_on_device)
{
    const int n = blockIdx.x * PT + threadIdx.x;
    if (n >= D.npoints || !D.pact[n]) return;
    const double lam = lambda_on_device ? D.sc[LM_SC_LAMBDA_INIT] : lambda;
    const double *blk = D.Hll + 12 * (size_t)n;
    double M[9], inv[9];
    ORBM_UNROLL for (int j = 0; j < 9; ++j) M[j] = blk[j];
    ORBM_UNROLL for (int j = 0; j < 3; ++j) M[4 * j] += lam;
    inverse3(M, inv);
    double *o = D.Dinv + 12 * (size_t)n;
    ORBM_UNROLL for (int j = 0; j < 9; ++j) o[j] = inv[j];
    ORBM_UNROLL for (int j = 0; j < 3; ++j) o[9 + j] = inv[3 * j] * blk[9] + inv[3 * j + 1] * blk[10] + inv[3 * j + 2] * blk[11];
}

// Entry (r, c) of block b = (i1 <= i2) of the free poses: Hpp (+ lambda on the diagonal) minus (B_i1 Dinv) B_i2^T, point after point
// over the block's entry list, edges off level 0 skipped.
__device__ __forceinline__ double ba_schur_entry(const BaDev &D, int b, int i1, int i2, int r, int c, double lam)
{
    double v = 0.0;
    if (i1 == i2) {
        const int hi = r > c ? r : c, lo = r > c ? c : r;
        v = D.Hpp[27 * i1 + hi * (hi + 1) / 2 + lo];
        if (r == c) v += lam;
    }
    for (int k = D.blk_start[b]; k < D.blk_start[b + 1]; ++k) {
        const int pt = D.blk_ent[3 * (size_t)k], e1 = D.blk_ent[3 * (size_t)k + 1], e2 = D.blk_ent[3 * (size_t)k + 2];
        if (D.e_level[e1] || D.e_level[e2]) continue;
        const double *h1 = D.Hpl + 18 * (size_t)e1 + 3 * r, *h2 = D.Hpl + 18 * (size_t)e2 + 3 * c, *inv = D.Dinv + 12 * (size_t)pt;
        const double w0 = h1[0] * inv[0] + h1[1] * inv[3] + h1[2] * inv[6];
        const double w1 = h1[0] * inv[1] + h1[1] * inv[4] + h1[2] * inv[7];
        const double w2 = h1[0] * inv[2] + h1[1] * inv[5] + h1[2] * inv[8];
        v -= w0 * h2[0] + w1 * h2[1] + w2 * h2[2];
    }
    return v;
}

// Row r of bschur of free pose i1, whose diagonal block is b: bp - sum B_i (Dinv bl) over the pose's edges (the diagonal block's
// entries are the pose's edge list, one for one)
__device__ __forceinline__ double ba_schur_rhs(const BaDev &D, int b, int i1, int r)
{
    double co = 0.0;
    for (int k = D.pe_start[i1]; k < D.pe_start[i1 + 1]; ++k) {
        const int e = D.pe_list[k];
        if (D.e_level[e]) continue;
        const double *h = D.Hpl + 18 * (size_t)e + 3 * r, *db = D.Dinv + 12 * (size_t)D.blk_ent[3 * ((size_t)D.blk_start[b] + (size_t)(k - D.pe_start[i1]))] + 9;
        co += h[0] * db[0] + h[1] * db[1] + h[2] * db[2];
    }
    return D.Hpp[27 * i1 + 21 + r] - co;
}

// One wave per upper block (i1 <= i2) of the free poses.  Lane 6 r + c owns entry (r, c) of the block; lanes 36 .. 41 of a diagonal
// block form bschur.
// The block's (i1, i2) is found by walking the rows: at most nfree steps (512, for the 131,328 blocks of the largest graph of
// orbm_global_bundle_adjustment), which is short beside the entry list of any block that has work.
__global__ __launch_bounds__(PT) void k_ba_schur(BaDev D, double lambda, int lambda_on_device)
{
    int i1 = 0, b = blockIdx.x;
    while (b >= D.nfree - i1) { b -= D.nfree - i1; ++i1; }
    const int i2 = i1 + b;
    const int r1 = D.ridx[i1], r2 = D.ridx[i2];
    if (r1 < 0 || r2 < 0) return;
    const double lam = lambda_on_device ? D.sc[LM_SC_LAMBDA_INIT] : lambda;
    const int n = 6 * D.isc[LM_ISC_NACT], l = threadIdx.x;
    if (l < 36) {
        const int r = l / 6, c = l % 6;
        const double v = ba_schur_entry(D, (int)blockIdx.x, i1, i2, r, c, lam);
        const int row = 6 * r2 + c, col = 6 * r1 + r;                   // the transposed entry: the lower triangle is what the LLT reads
        if (row >= col) D.S[(size_t)col * n + row] = v;
    } else if (l < 42 && i1 == i2)
        D.bsch[6 * r1 + l - 36] = ba_schur_rhs(D, (int)blockIdx.x, i1, l - 36);
}

// The same entries for LISTED block blockIdx.x of the compact list (orbm_global_bundle_adjustment_env): (i1, i2) come from the list,
// and the transposed entry with row >= col goes into packed tile off[R] + C - first[R] of the envelope, column-major.  T is no
// multiple of 6, so a block may reach into two row tiles and two column tiles.  The host took first[] from the same list and the
// same ridx, so C >= first[R] holds for every entry; the test keeps a write inside its own row tile's span whatever happens.
__global__ __launch_bounds__(PT) void k_ba_schur_env(BaDev D, double lambda, int lambda_on_device)
{
    const int b = blockIdx.x, i1 = D.blk_i1[b], i2 = D.blk_i2[b];
    const int r1 = D.ridx[i1], r2 = D.ridx[i2];
    if (r1 < 0 || r2 < 0) return;
    const double lam = lambda_on_device ? D.sc[LM_SC_LAMBDA_INIT] : lambda;
    const int l = threadIdx.x;
    if (l < 36) {
        const int r = l / 6, c = l % 6;
        const double v = ba_schur_entry(D, b, i1, i2, r, c, lam);
        const int row = 6 * r2 + c, col = 6 * r1 + r, T = D.T;
        const int R = row / T, C = col / T;
        const LltEnvView env(D.env, D.nt);
        if (row >= col && R < D.nt && C >= env.first[R]) D.A[((size_t)env.tile_index(R, C) * T + (size_t)(col - C * T)) * T + (size_t)(row - R * T)] = v;
    } else if (l < 42 && i1 == i2)
        D.bsch[6 * r1 + l - 36] = ba_schur_rhs(D, b, i1, l - 36);
}

// Dense LLT of the reduced system and the two triangular solves.  Thread i owns row i.  L[i][j] = (a[i][j] - sum_{k < j} L[i][k]
// L[j][k]) / L[j][j], the sum from k = 0 upwards; a pivot <= 0 (or NaN) ends it with ok2 = 0.
__global__ __launch_bounds__(ST) void k_ba_solve(BaDev D)
{
    __shared__ double s_row[ST];
    __shared__ double s_b[2];
    __shared__ int s_ok;
    const int n = 6 * D.isc[LM_ISC_NACT], i = threadIdx.x;
    double *S = D.S;
    if (i == 0) s_ok = 1;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        for (int k = i; k < j; k += ST) s_row[k] = S[(size_t)k * n + j];
        __syncthreads();
        double s = 0.0;
        if (i >= j && i < n) {
            s = S[(size_t)j * n + i];
            if (j > 0) {
                double dot = S[i] * s_row[0];
                for (int k = 1; k < j; ++k) dot = dot + S[(size_t)k * n + i] * s_row[k];
                s = s - dot;
            }
        }
        if (i == j) {
            if (s > 0.0) { s = sqrt(s); S[(size_t)j * n + j] = s; s_b[0] = s; }
            else s_ok = 0;
        }
        __syncthreads();
        if (!s_ok) break;
        if (i > j && i < n) S[(size_t)j * n + i] = s / s_b[0];
        __syncthreads();
    }
    const bool ok = s_ok != 0;
    if (i == 0) D.isc[LM_ISC_OK2] = ok ? 1 : 0;
    if (!ok) {
        if (i < n) D.xp[i] = 0.0;
        return;
    }
    double y = i < n ? D.bsch[i] : 0.0;
    for (int j = 0; j < n; ++j) {                               // L y = b, column after column
        if (i == j) { y = y / S[(size_t)j * n + j]; s_b[j & 1] = y; }
        __syncthreads();
        if (i > j && i < n) y -= S[(size_t)j * n + i] * s_b[j & 1];
    }
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {                          // L^T x = y
        if (i == j) { y = y / S[(size_t)j * n + j]; s_b[j & 1] = y; }
        __syncthreads();
        if (i < j) y -= S[(size_t)i * n + j] * s_b[j & 1];
    }
    if (i < n) D.xp[i] = y;
}

// push; xl = Dinv (bl - B^T xp); oplus on the points; the points' terms of computeScale
__global__ __launch_bounds__(PT) void k_ba_update(BaDev D, double lambda, int lambda_on_device)
{
    const int n = blockIdx.x * PT + threadIdx.x;
    double sc = 0.0;
    if (n < D.npoints) {
        double X[3] = {D.X[3 * (size_t)n], D.X[3 * (size_t)n + 1], D.X[3 * (size_t)n + 2]};
        ORBM_UNROLL for (int j = 0; j < 3; ++j) D.X_bak[3 * (size_t)n + j] = X[j];
        if (D.pact[n] && D.isc[LM_ISC_OK2]) {
            const double lam = lambda_on_device ? D.sc[LM_SC_LAMBDA_INIT] : lambda;
            const double *blk = D.Hll + 12 * (size_t)n, *inv = D.Dinv + 12 * (size_t)n;
            double cl[3] = {blk[9], blk[10], blk[11]};
            for (int e = D.e_start[n]; e < D.e_start[n + 1]; ++e) {
                if (D.e_level[e]) continue;
                const int cam = D.e_cam[e];
                if (cam >= D.nfree) continue;
                const int r = D.ridx[cam];
                if (r < 0) continue;
                const double *hp = D.Hpl + 18 * (size_t)e, *x = D.xp + 6 * r;
                ORBM_UNROLL for (int q = 0; q < 6; ++q) {
                    const double cp = -x[q];
                    ORBM_UNROLL for (int j = 0; j < 3; ++j) cl[j] = cl[j] + hp[3 * q + j] * cp;
                }
            }
            ORBM_UNROLL for (int j = 0; j < 3; ++j) {
                const double dx = inv[3 * j] * cl[0] + inv[3 * j + 1] * cl[1] + inv[3 * j + 2] * cl[2];
                D.X[3 * (size_t)n + j] = X[j] + dx;
                sc += dx * (lam * dx + blk[9 + j]);
            }
        }
    }
    sc = wave_sum(sc);
    if (threadIdx.x == 0) D.part_scale[blockIdx.x] = sc;
}

// push; SE3Quat::exp(update) * estimate; a pose's terms of computeScale.  A thread per free pose.
__global__ __launch_bounds__(PT) void k_ba_update_pose(BaDev D, double lambda, int lambda_on_device)
{
    const int p = blockIdx.x * PT + threadIdx.x;
    if (p >= D.nfree) return;
    Se3 T;
    load_pose(D.est, p, T);
    store_pose(D.est_bak, p, T);
    double sc = 0.0;
    const int r = D.ridx[p];
    if (r >= 0 && D.isc[LM_ISC_OK2]) {
        const double lam = lambda_on_device ? D.sc[LM_SC_LAMBDA_INIT] : lambda;
        double x[6];
        ORBM_UNROLL for (int j = 0; j < 6; ++j) x[j] = D.xp[6 * r + j];
        Se3 up, o;
        se3_exp(x, up);
        se3_compose(up, T, o);
        store_pose(D.est, p, o);
        ORBM_UNROLL for (int j = 0; j < 6; ++j) sc += x[j] * (lam * x[j] + D.Hpp[27 * p + 21 + j]);
    }
    D.pose_scale[p] = sc;
}

__global__ __launch_bounds__(PT) void k_ba_pop(BaDev D)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < D.nfree)
        for (int j = 0; j < 7; ++j) D.est[7 * i + j] = D.est_bak[7 * i + j];
    if (i < D.npoints)
        for (int j = 0; j < 3; ++j) D.X[3 * (size_t)i + j] = D.X_bak[3 * (size_t)i + j];
}

// Optimizer.cc:1051-1087 (final = 0: level 1) and :1091-1127 (final = 1: vToErase): chi2() of the STORED error, isDepthPositive()
// at the CURRENT estimates
__global__ __launch_bounds__(PT) void k_ba_classify(BaDev D, double chi2_mono, double chi2_stereo, int final)
{
    const int n = blockIdx.x * PT + threadIdx.x;
    if (n >= D.npoints) return;
    const double X[3] = {D.X[3 * (size_t)n], D.X[3 * (size_t)n + 1], D.X[3 * (size_t)n + 2]};
    for (int e = D.e_start[n]; e < D.e_start[n + 1]; ++e) {
        const double err[3] = {D.e_err[3 * (size_t)e], D.e_err[3 * (size_t)e + 1], D.e_err[3 * (size_t)e + 2]};
        const double c2 = ba_chi2(err, (double)D.e_info[e]);
        Se3 T;
        load_pose(D.est, D.e_cam[e], T);
        double c[3];
        se3_map(T, X, c);
        const bool bad = c2 > (D.e_obs[3 * (size_t)e + 2] < 0.f ? chi2_mono : chi2_stereo) || !(c[2] > 0.0);
        if (final) D.erase[e] = bad;
        else if (bad) D.e_level[e] = 1;
    }
}

// write-back: Converter::toCvMat of the poses and of the points; the stored chi2 and the level of every edge
__global__ __launch_bounds__(PT) void k_ba_final(BaDev D)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < D.nfree) {
        Se3 T;
        load_pose(D.est, i, T);
        float *o = D.poses_out + 16 * (size_t)i;
        double R[9];                                            // (every local keyframe, the fixed one included: :1146-1152)
        quat_to_matrix(T.q, R);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)R[3 * r + c];
            o[4 * r + 3] = (float)T.t[r];
        }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
        for (int j = 0; j < 7; ++j) D.poses_d[7 * (size_t)i + j] = D.est[7 * (size_t)i + j];
    }
    if (i < D.npoints)
        for (int j = 0; j < 3; ++j) {
            const bool connected = D.e_start[i + 1] > D.e_start[i];
            D.points_out[3 * (size_t)i + j] = connected ? (float)D.X[3 * (size_t)i + j] : D.points_in[3 * (size_t)i + j];
            D.points_d[3 * (size_t)i + j] = D.X[3 * (size_t)i + j];
        }
    if (i < D.nedges) {
        const double err[3] = {D.e_err[3 * (size_t)i], D.e_err[3 * (size_t)i + 1], D.e_err[3 * (size_t)i + 2]};
        D.chi2_out[i] = ba_chi2(err, (double)D.e_info[i]);
        D.level_out[i] = D.e_level[i];
    }
}

// ---- host

struct BaPlan {
    std::vector<int32_t> e_start, pose_class, point_class, pe_start, pe_list, blk_start, blk_ent;
    std::vector<int32_t> blk_i1, blk_i2;        // BA_ENV: the listed blocks; blk_start then has one entry per listed block, and one more
};

inline int block_index(int nfree, int i1, int i2) { return i1 * nfree - i1 * (i1 - 1) / 2 + (i2 - i1); }

// limits, indices, grouping; the vertex classes, the pose -> edge lists and the block -> (point, edge, edge) lists
int ba_plan(const orbm_ba_graph &g, BaPlan &P, int mode)
{
    const bool env = mode == BA_ENV;
    if (g.nfree < 0 || g.nfixed < 0 || g.npoints < 0 || g.nedges < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative size");
    if (mode == BA_LOCAL && g.nfree > BA_MAXFREE) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 64 free keyframes");
    if (mode == BA_GLOBAL && g.nfree > BA_MAXFREE_GLOBAL) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 512 free keyframes");
    if (env && g.nfree > BA_MAXFREE_ENV) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 4,096 free keyframes");
    if (g.nfixed > BA_MAXFIXED) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,024 fixed keyframes");
    if (!env && g.npoints > BA_MAXPOINTS) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 65,536 points");
    if (!env && g.nedges > BA_MAXEDGES) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 524,288 edges");
    if (env && g.npoints > BA_MAXPOINTS_ENV) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,048,576 points");
    if (env && g.nedges > BA_MAXEDGES_ENV) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 4,194,304 edges");
    const int npose = g.nfree + g.nfixed;
    if ((npose && !g.poses) || (g.npoints && !g.points) || (g.nedges && (!g.e_point || !g.e_cam || !g.e_obs || !g.e_inv_sigma2 || !g.e_cam_k)))
        ORBX_FAIL(ORBX_ERR_ARG, "null pointer in the graph");
    P.e_start.assign((size_t)g.npoints + 1, 0);
    P.pose_class.assign((size_t)npose, 2);
    P.point_class.assign((size_t)g.npoints, 1);
    for (int p = g.nfree; p < npose; ++p) P.pose_class[p] = 1;
    for (int p = 0; p < g.nfree; ++p)
        if (g.fixed && g.fixed[p]) P.pose_class[p] = 1;
    int prev = 0;
    for (int e = 0; e < g.nedges; ++e) {
        const int p = g.e_point[e], c = g.e_cam[e];
        if (p < 0 || p >= g.npoints) ORBX_FAIL(ORBX_ERR_ARG, "an edge's point index is out of range");
        if (c < 0 || c >= npose) ORBX_FAIL(ORBX_ERR_ARG, "an edge's keyframe index is out of range");
        if (p < prev) ORBX_FAIL(ORBX_ERR_ARG, "edges must be grouped by point, points ascending");
        prev = p;
        P.e_start[(size_t)p + 1]++;
        P.point_class[p] = 0;
        if (P.pose_class[c] == 2) P.pose_class[c] = 0;
    }
    for (int n = 0; n < g.npoints; ++n) P.e_start[(size_t)n + 1] += P.e_start[n];
    // a keyframe observes a point once
    {
        std::vector<int32_t> seen((size_t)npose, -1);
        for (int e = 0; e < g.nedges; ++e) {
            if (seen[g.e_cam[e]] == g.e_point[e]) ORBX_FAIL(ORBX_ERR_ARG, "a keyframe observes a point twice");
            seen[g.e_cam[e]] = g.e_point[e];
        }
    }
    auto is_free = [&](int c) { return c < g.nfree && P.pose_class[c] == 0; };
    int64_t nentries = 0;
    if (mode != BA_LOCAL) {                                             // the block lists' size, before they are counted block by block
        int64_t entries = 0;
        for (int n = 0; n < g.npoints; ++n) {
            int64_t d = 0;
            for (int a = P.e_start[n]; a < P.e_start[n + 1]; ++a) d += is_free(g.e_cam[a]);
            entries += d * (d + 1) / 2;
        }
        if (!env && entries > BA_MAXBLOCKENT_GLOBAL) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "the block lists exceed 2^25 entries");
        if (env && entries > BA_MAXBLOCKENT_ENV) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "the block lists exceed 2^26 entries");
        nentries = entries;
    }
    const int nblk = env ? 0 : g.nfree * (g.nfree + 1) / 2;                 // (the env entry has no dense block index)
    P.pe_start.assign((size_t)g.nfree + 1, 0);
    P.blk_start.assign(env ? 0 : (size_t)nblk + 1, 0);
    for (int n = 0; n < g.npoints; ++n)
        for (int a = P.e_start[n]; a < P.e_start[n + 1]; ++a) {
            const int ca = g.e_cam[a];
            if (!is_free(ca)) continue;
            P.pe_start[(size_t)ca + 1]++;
            for (int b = P.e_start[n]; b < P.e_start[n + 1] && !env; ++b) {
                const int cb = g.e_cam[b];
                if (!is_free(cb) || cb < ca) continue;
                P.blk_start[(size_t)block_index(g.nfree, ca, cb) + 1]++;
            }
        }
    for (int p = 0; p < g.nfree; ++p) P.pe_start[(size_t)p + 1] += P.pe_start[p];
    for (int b = 0; b < nblk; ++b) {
        if ((int64_t)P.blk_start[(size_t)b + 1] + P.blk_start[b] > 0x7fffffff / 3) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "the block lists exceed 2^31 entries");
        P.blk_start[(size_t)b + 1] += P.blk_start[b];
    }
    P.pe_list.assign((size_t)P.pe_start[g.nfree], 0);
    P.blk_ent.assign(env ? 0 : 3 * (size_t)P.blk_start[nblk], 0);
    std::vector<int32_t> pe_fill(P.pe_start.begin(), P.pe_start.end() - 1), blk_fill(P.blk_start.begin(), P.blk_start.end() - (env ? 0 : 1));
    for (int n = 0; n < g.npoints; ++n)
        for (int a = P.e_start[n]; a < P.e_start[n + 1]; ++a) {
            const int ca = g.e_cam[a];
            if (!is_free(ca)) continue;
            P.pe_list[(size_t)pe_fill[ca]++] = a;
            for (int b = P.e_start[n]; b < P.e_start[n + 1] && !env; ++b) {
                const int cb = g.e_cam[b];
                if (!is_free(cb) || cb < ca) continue;
                int32_t *o = &P.blk_ent[3 * (size_t)blk_fill[block_index(g.nfree, ca, cb)]++];
                o[0] = n; o[1] = a; o[2] = b;
            }
        }
    if (!env) return ORBX_OK;
    // The compact list: the non-empty blocks alone, sorted by (i1, i2).  Row i1's entries are found from the pose's edge list (edges
    // ascending, so points ascending) and sorted by i2 in a stable sort: a block's entries keep the dense lists' order.
    struct Ent { int32_t i2, n, a, b; };
    std::vector<Ent> row;
    P.blk_ent.reserve(3 * (size_t)nentries);
    for (int i1 = 0; i1 < g.nfree; ++i1) {
        row.clear();
        for (int k = P.pe_start[i1]; k < P.pe_start[i1 + 1]; ++k) {
            const int a = P.pe_list[k], n = g.e_point[a];
            for (int b = P.e_start[n]; b < P.e_start[n + 1]; ++b)
                if (is_free(g.e_cam[b]) && g.e_cam[b] >= i1) row.push_back({g.e_cam[b], n, a, b});
        }
        std::stable_sort(row.begin(), row.end(), [](const Ent &x, const Ent &y) { return x.i2 < y.i2; });
        for (size_t k = 0; k < row.size(); ++k) {
            if (k == 0 || row[k].i2 != row[k - 1].i2) {
                P.blk_i1.push_back(i1); P.blk_i2.push_back(row[k].i2);
                P.blk_start.push_back((int32_t)(P.blk_ent.size() / 3));
            }
            P.blk_ent.push_back(row[k].n); P.blk_ent.push_back(row[k].a); P.blk_ent.push_back(row[k].b);
        }
    }
    P.blk_start.push_back((int32_t)(P.blk_ent.size() / 3));
    return ORBX_OK;
}

// The tile envelope of the reduced system of one round, and what orbm_llt_env_solve_dev reads on the device.  ridx[nfree]: a pose's
// row block in the round's system, or -1.  Listed block (i1 <= i2) covers rows 6 r2 .. 6 r2 + 5 from column 6 r1: first[R] is the
// smallest column tile over the blocks that reach row tile R, and R where none does.  The block STRUCTURE decides, not the edge
// levels: a superset, exactly zero where the levels mask.  Refuses as orbm_llt_env_plan does (more than 8,192 live tiles).
int ba_env_plan(const BaPlan &P, const int32_t *ridx, int nact, LltEnvPlan &E)
{
    const int T = orbm_llt_tile();
    llt_env_start(E, 6 * nact);
    if (nact == 0) return ORBX_OK;                                  // no row tile: first[] is empty and nothing may reach into it
    for (size_t b = 0; b < P.blk_i1.size(); ++b) {
        const int r1 = ridx[P.blk_i1[b]], r2 = ridx[P.blk_i2[b]];
        if (r1 >= 0 && r2 >= 0) llt_env_reach(E.first, T, 6 * r2, 6 * r2 + 5, 6 * r1);
    }
    return llt_env_finish(E);
}

// round 0's system: every free, connected keyframe, in the caller's order (what k_ba_activate finds with every edge on level 0)
int round0_rows(const orbm_ba_graph &g, const BaPlan &P, std::vector<int32_t> &ridx)
{
    int r = 0;
    ridx.assign((size_t)g.nfree, -1);
    for (int p = 0; p < g.nfree; ++p)
        if (P.pose_class[p] == 0) ridx[(size_t)p] = r++;
    return r;
}

int check_options(const orbm_ba_options &o)
{
    if (o.nrounds < 1 || o.nrounds > 2) ORBX_FAIL(ORBX_ERR_ARG, "nrounds must be 1 or 2");
    for (int r = 0; r < 2; ++r)
        if (o.iterations[r] < 0 || o.iterations[r] > BA_MAXITER) ORBX_FAIL(ORBX_ERR_ARG, "iterations outside 0 .. 64");
    if ((o.robust_round0 != 0 && o.robust_round0 != 1) || (o.classify != 0 && o.classify != 1)) ORBX_FAIL(ORBX_ERR_ARG, "robust_round0 and classify are 0 or 1");
    if (!(o.huber_mono > 0) || !(o.huber_stereo > 0) || !(o.chi2_mono > 0) || !(o.chi2_stereo > 0) || !std::isfinite(o.huber_mono) ||
        !std::isfinite(o.huber_stereo) || !std::isfinite(o.chi2_mono) || !std::isfinite(o.chi2_stereo))
        ORBX_FAIL(ORBX_ERR_ARG, "the Huber deltas and chi2 thresholds must be positive and finite");
    return ORBX_OK;
}

std::atomic<int> g_last_ba_waits{0};    // host waits of the last orbm_bundle_adjustment / orbm_global_bundle_adjustment of this process

void reset_stats(orbm_ba_stats *st)
{
    if (!st) return;
    st->rounds = 0;
    for (int r = 0; r < 2; ++r) { st->iterations[r] = 0; st->trials[r] = 0; }
    st->nresults = 0;
    for (int j = 0; j < 128; ++j) st->results[j] = 0;
    st->ntrials = 0; st->trial_overflow = 0;
}

// nothing to optimise, or stopped before the first optimize: the input comes back
void answer_unchanged(const orbm_ba_graph &g, const orbm_ba_options &opt, const BaPlan &P, orbm_ba_result &out, orbm_ba_stats *st, int stopped)
{
    if (g.nfree) memcpy(out.poses, g.poses, sizeof(float) * 16 * (size_t)g.nfree);
    if (g.npoints) memcpy(out.points, g.points, sizeof(float) * 3 * (size_t)g.npoints);
    if (opt.classify && out.erase) memset(out.erase, 0, (size_t)g.nedges);
    for (int n = 0; out.not_included && n < g.npoints; ++n) out.not_included[n] = (uint8_t)P.point_class[n];
    out.stopped = stopped;
    reset_stats(st);
}

int plan_out(const orbm_ba_graph *g, int mode, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
             int32_t *block_start, int32_t *block_entries, int32_t *counts)
{
    if (!g) ORBX_FAIL(ORBX_ERR_ARG, "null graph");
    BaPlan P;
    const int rc = ba_plan(*g, P, mode);
    if (rc != ORBX_OK) return rc;
    auto copy = [](int32_t *dst, const std::vector<int32_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    copy(pose_class, P.pose_class); copy(point_class, P.point_class); copy(pose_edge_start, P.pe_start); copy(pose_edges, P.pe_list);
    copy(block_start, P.blk_start); copy(block_entries, P.blk_ent);
    if (counts) { counts[0] = (int32_t)P.pe_list.size(); counts[1] = (int32_t)(P.blk_ent.size() / 3); }
    return ORBX_OK;
}

// The body of the three public entries.  BA_GLOBAL: the limits of orbm_global_bundle_adjustment and the tiled solve (orbm_llt_solve_dev over
// the arena's S, bschur, xp and the trial block's ok2 word) in k_ba_solve's place, at every size.  BA_ENV: the limits of
// orbm_global_bundle_adjustment_env, the compact block list, the live tiles A (zeroed, then k_ba_schur_env) with the solver's W in
// S's place, orbm_llt_env_solve_dev at every size, and between the rounds ridx[] in the read-back, the envelope planned again on the
// host and its image uploaded.  results[128] holds for all: an iteration writes one, and two rounds of at most 64 make 128.
int ba_run(const orbm_ba_graph *gp, const orbm_ba_options *op, const volatile uint8_t *stop_flag, orbm_ba_result *outp, orbm_ba_stats *stats,
           int mode)
{
    if (!gp || !op || !outp) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    const orbm_ba_graph &g = *gp;
    const orbm_ba_options &opt = *op;
    orbm_ba_result &out = *outp;
    const bool env = mode == BA_ENV;
    BaPlan P;
    LltEnvPlan E;
    int rc = ba_plan(g, P, mode);
    if (rc != ORBX_OK) return rc;
    if ((rc = check_options(opt)) != ORBX_OK) return rc;
    if ((g.nfree && !out.poses) || (g.npoints && !out.points) || (opt.classify && g.nedges && !out.erase)) ORBX_FAIL(ORBX_ERR_ARG, "null result array");
    if (stats && stats->trial_capacity < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative trial capacity");
    if (stats && stats->trial_capacity > 0 && !stats->trial_log) ORBX_FAIL(ORBX_ERR_ARG, "trial capacity without a trial log");
    if (env) {                                                                  // round 0's tile cap, behind every argument check
        std::vector<int32_t> ridx0;
        const int nact0 = round0_rows(g, P, ridx0);
        if ((rc = ba_env_plan(P, ridx0.data(), nact0, E)) != ORBX_OK) return rc;
    }
    bool stop_seen = false;
    auto terminate = [&]() { if (stop_flag && *stop_flag) stop_seen = true; return stop_seen && stop_flag && *stop_flag; };
    g_last_ba_waits = 0;
    int nact = 0, nactive_edges = g.nedges;
    for (int p = 0; p < g.nfree; ++p) nact += P.pose_class[p] == 0;
    if (g.nfree == 0 || g.nedges == 0 || nact == 0) {
        answer_unchanged(g, opt, P, out, stats, 0);
        for (int i = 0; stats && stats->poses && i < 7 * g.nfree; ++i) stats->poses[i] = 0.0;
        for (int i = 0; stats && stats->points && i < 3 * g.npoints; ++i) stats->points[i] = (double)g.points[i];
        for (int i = 0; stats && stats->chi2 && i < g.nedges; ++i) stats->chi2[i] = 0.0;
        for (int i = 0; stats && stats->level && i < g.nedges; ++i) stats->level[i] = 0;
        return ORBX_OK;
    }
    if (terminate()) {                                                          // Optimizer.cc:1039-1041
        answer_unchanged(g, opt, P, out, stats, 1);
        return ORBX_OK;
    }
    ORBX_NEED_DEVICE();

    // (with its initialiser: the lease-site table of tests/workspace_cases.py lists the calls whose stale-arena case lives there; this
    // call's case is tests/test_gpu_ba_workspace.py, and tests/test_cpu_ba.py holds the two together)
    StagedCall sc{};
    BaDev D;
    memset(&D, 0, sizeof(D));
    const size_t npose = (size_t)g.nfree + g.nfixed, np = (size_t)g.npoints, ne = (size_t)g.nedges, nf = (size_t)g.nfree;
    const size_t nblk = (np + PT - 1) / PT, nmax = 6 * nf;
    D.nfree = g.nfree; D.npose = (int)npose; D.npoints = g.npoints; D.nedges = g.nedges; D.nblocks = (int)nblk;
    const size_t o_poses = sc.in(g.poses, sizeof(float) * 16 * npose), o_points = sc.in(g.points, sizeof(float) * 3 * np);
    const size_t o_obs = sc.in(g.e_obs, sizeof(float) * 3 * ne), o_info = sc.in(g.e_inv_sigma2, sizeof(float) * ne), o_K = sc.in(g.e_cam_k, sizeof(float) * 5 * ne);
    const size_t o_cam = sc.in(g.e_cam, sizeof(int32_t) * ne), o_es = sc.in(P.e_start.data(), sizeof(int32_t) * (np + 1));
    const size_t o_pc = sc.in(P.pose_class.data(), sizeof(int32_t) * npose), o_ps = sc.in(P.pe_start.data(), sizeof(int32_t) * (nf + 1));
    const size_t o_pl = sc.in(P.pe_list.data(), sizeof(int32_t) * P.pe_list.size()), o_bs = sc.in(P.blk_start.data(), sizeof(int32_t) * P.blk_start.size());
    const size_t o_be = sc.in(P.blk_ent.data(), sizeof(int32_t) * P.blk_ent.size());
    // BA_ENV: the block list's (i1, i2); room for the largest plan image a round of this call can have; the live tiles twice.  A
    // second round's rows are the first's with some keyframes left out: an old row tile's rows land in at most two new ones and no
    // entry moves further from the diagonal, so 2 live + nt tiles hold any second round (the solver's own cap aside).
    const size_t Tt = (size_t)orbm_llt_tile(), nlisted = P.blk_i1.size();
    const size_t tile_cap = !env ? 0 : opt.nrounds == 1 ? (size_t)E.live : std::min(std::min(2 * (size_t)E.live + (size_t)E.nt, (size_t)E.nt * ((size_t)E.nt + 1) / 2), (size_t)BA_ENV_MAXTILES);
    const size_t image_cap = sizeof(int32_t) * LltEnvView::words((size_t)E.nt, tile_cap);
    const size_t o_bi1 = env ? sc.in(P.blk_i1.data(), sizeof(int32_t) * nlisted) : 0, o_bi2 = env ? sc.in(P.blk_i2.data(), sizeof(int32_t) * nlisted) : 0;
    const size_t o_env = env ? sc.in(nullptr, image_cap) : 0;
    if (env) sc.in_at(o_env, E.image.data(), sizeof(int32_t) * E.image.size());
    const size_t o_est = sc.scratch(sizeof(double) * 7 * npose), o_estb = sc.scratch(sizeof(double) * 7 * nf);
    const size_t o_X = sc.scratch(sizeof(double) * 3 * np), o_Xb = sc.scratch(sizeof(double) * 3 * np), o_err = sc.scratch(sizeof(double) * 3 * ne);
    const size_t o_Hll = sc.scratch(sizeof(double) * 12 * np), o_Dinv = sc.scratch(sizeof(double) * 12 * np);
    const size_t o_Hpl = sc.scratch(sizeof(double) * 18 * ne), o_cb = sc.scratch(sizeof(double) * 27 * ne), o_Hpp = sc.scratch(sizeof(double) * 27 * nf);
    const size_t o_pm = sc.scratch(sizeof(double) * nf), o_psc = sc.scratch(sizeof(double) * nf);
    const size_t o_S = sc.scratch(env ? 0 : sizeof(double) * nmax * nmax), o_bsch = sc.scratch(sizeof(double) * nmax), o_xp = sc.scratch(sizeof(double) * nmax);
    const size_t o_pchi = sc.scratch(sizeof(double) * nblk), o_pmax = sc.scratch(sizeof(double) * nblk), o_pscale = sc.scratch(sizeof(double) * nblk);
    const size_t o_lvl = sc.scratch(ne), o_pact = sc.scratch(np);
    const size_t o_A = env ? sc.scratch(sizeof(double) * tile_cap * Tt * Tt) : 0, o_W = env ? sc.scratch(sizeof(double) * tile_cap * Tt * Tt) : 0;
    size_t o_ridx = env ? 0 : sc.scratch(sizeof(int) * nf);
    const size_t o_sc = sc.out(LM_BLOCK_BYTES);                                 // what a trial reads back
    if (env) o_ridx = sc.out(sizeof(int) * nf);                                 // BA_ENV: behind it, so that a round's read-back brings the rows too
    const size_t round_head = env ? o_ridx + sizeof(int) * nf - o_sc : LM_BLOCK_BYTES;
    if (env && o_env < round_head) ORBX_FAIL(ORBX_ERR_ARG, "internal: the plan image overlaps the round's read-back");   // (the inputs in front of it are longer)
    const size_t o_pout = sc.out(sizeof(float) * 16 * nf), o_xout = sc.out(sizeof(float) * 3 * np), o_erase = sc.out(ne), o_lout = sc.out(ne);
    const size_t o_chi = sc.out(sizeof(double) * ne), o_pd = sc.out(sizeof(double) * 7 * nf), o_xd = sc.out(sizeof(double) * 3 * np);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    D.poses_in = sc.d<float>(o_poses); D.points_in = sc.d<float>(o_points); D.e_obs = sc.d<float>(o_obs); D.e_info = sc.d<float>(o_info);
    D.e_K = sc.d<float>(o_K); D.e_cam = sc.d<int>(o_cam); D.e_start = sc.d<int>(o_es); D.pose_class = sc.d<int>(o_pc);
    D.pe_start = sc.d<int>(o_ps); D.pe_list = sc.d<int>(o_pl); D.blk_start = sc.d<int>(o_bs); D.blk_ent = sc.d<int>(o_be);
    D.est = sc.d<double>(o_est); D.est_bak = sc.d<double>(o_estb); D.X = sc.d<double>(o_X); D.X_bak = sc.d<double>(o_Xb);
    D.e_err = sc.d<double>(o_err); D.Hll = sc.d<double>(o_Hll); D.Dinv = sc.d<double>(o_Dinv); D.Hpl = sc.d<double>(o_Hpl);
    D.contrib = sc.d<double>(o_cb); D.Hpp = sc.d<double>(o_Hpp); D.pose_max = sc.d<double>(o_pm); D.pose_scale = sc.d<double>(o_psc);
    D.S = sc.d<double>(o_S); D.bsch = sc.d<double>(o_bsch); D.xp = sc.d<double>(o_xp);
    D.part_chi = sc.d<double>(o_pchi); D.part_max = sc.d<double>(o_pmax); D.part_scale = sc.d<double>(o_pscale);
    D.e_level = sc.d<uint8_t>(o_lvl); D.pact = sc.d<uint8_t>(o_pact); D.ridx = sc.d<int>(o_ridx);
    D.sc = sc.d<double>(o_sc); D.isc = reinterpret_cast<int *>(sc.d<double>(o_sc) + 8);
    D.poses_out = sc.d<float>(o_pout); D.points_out = sc.d<float>(o_xout); D.erase = sc.d<uint8_t>(o_erase); D.level_out = sc.d<uint8_t>(o_lout);
    D.chi2_out = sc.d<double>(o_chi); D.poses_d = sc.d<double>(o_pd); D.points_d = sc.d<double>(o_xd);
    if (env) {
        D.blk_i1 = sc.d<int>(o_bi1); D.blk_i2 = sc.d<int>(o_bi2); D.env = sc.d<int>(o_env); D.A = sc.d<double>(o_A); D.W = sc.d<double>(o_W);
        D.T = (int)Tt; D.nt = E.nt;
    }

    hipStream_t st = sc.stream();
    const size_t nall = std::max(std::max(npose, np), ne);
    const dim3 g_all((unsigned)((nall + PT - 1) / PT)), g_pts((unsigned)nblk), b_pt(PT);
    const unsigned nblocks_schur = (unsigned)(g.nfree * (g.nfree + 1) / 2);
    LmHostLoop L{sc, stats ? stats->trial_log : nullptr, stats ? stats->trial_capacity : 0};

    hipLaunchKernelGGL(k_ba_init, g_all, b_pt, 0, st, D);
    hipLaunchKernelGGL(k_ba_activate, dim3(1), dim3(RT), 0, st, D);
    reset_stats(stats);
    const double dm = opt.huber_mono, ds = opt.huber_stereo;
    int stopped = 0, nr = 0, rounds_run = 0;
    int st_iter[2] = {0, 0}, st_trials[2] = {0, 0};
    for (int round = 0; round < opt.nrounds; ++round) {
        const int robust = round == 0 && opt.robust_round0;
        bool ok = true;
        if (nact > 0 && nactive_edges > 0) {
            ++rounds_run;
            for (int it = 0; it < opt.iterations[round] && !terminate() && ok; ++it) {      // SparseOptimizer::optimize
                hipLaunchKernelGGL(k_ba_errors, g_pts, b_pt, 0, st, D, robust, dm, ds);
                hipLaunchKernelGGL(k_ba_build, g_pts, b_pt, 0, st, D, robust, dm, ds);
                hipLaunchKernelGGL(k_ba_pose, dim3((unsigned)g.nfree), b_pt, 0, st, D);
                hipLaunchKernelGGL(k_ba_reduce, dim3(1), dim3(RT), 0, st, D, 0);
                // (the first trial of an optimize() call runs at computeLambdaInit's value, which is still on the device: its
                // read-back brings the iteration's chi2 and that lambda, levenberg.cpp:97-115)
                auto on_dev = [&]() { return it == 0 && L.qmax == 0; };
                auto trial = [&](double lambda) -> int {
                    const int od = on_dev();
                    hipLaunchKernelGGL(k_ba_dinv, g_pts, b_pt, 0, st, D, lambda, od);
                    if (env) {                                                  // the factorisation has overwritten the live tiles, and the solver reads every entry of one
                        ORBX_HIP(hipMemsetAsync(D.A, 0, sizeof(double) * (size_t)E.live * Tt * Tt, st));
                        hipLaunchKernelGGL(k_ba_schur_env, dim3((unsigned)nlisted), b_pt, 0, st, D, lambda, od);
                        if (const int e = orbm_llt_env_solve_dev(6 * nact, E.first.data(), D.env, D.A, D.W, D.bsch, D.xp, D.isc + LM_ISC_OK2, st)) return e;
                    } else {
                        hipLaunchKernelGGL(k_ba_schur, dim3(nblocks_schur), b_pt, 0, st, D, lambda, od);
                        if (mode == BA_LOCAL) hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(ST), 0, st, D);
                        else if (const int e = orbm_llt_solve_dev(6 * nact, D.S, D.bsch, D.xp, D.isc + LM_ISC_OK2, st)) return e;   // nact: what k_ba_activate left in isc[LM_ISC_NACT]
                    }
                    hipLaunchKernelGGL(k_ba_update, g_pts, b_pt, 0, st, D, lambda, od);
                    hipLaunchKernelGGL(k_ba_update_pose, dim3((unsigned)((g.nfree + PT - 1) / PT)), b_pt, 0, st, D, lambda, od);
                    hipLaunchKernelGGL(k_ba_errors, g_pts, b_pt, 0, st, D, robust, dm, ds);
                    hipLaunchKernelGGL(k_ba_reduce, dim3(1), dim3(RT), 0, st, D, 1);
                    return ORBX_OK;
                };
                auto after_read = [&]() {
                    if (!on_dev()) return;
                    L.currentChi = L.iniChi = L.scalar(LM_SC_CHI2);
                    L.lm.start(L.scalar(LM_SC_LAMBDA_INIT));
                };
                auto pop = [&]() { hipLaunchKernelGGL(k_ba_pop, g_all, b_pt, 0, st, D); };
                if ((rc = L.trials(round, trial, after_read, pop, terminate)) != ORBX_OK) return rc;
                st_iter[round]++;
                st_trials[round] += L.qmax;
                const int result = L.lm.end_iteration(L.qmax, L.rho, L.iniChi, L.currentChi);
                if (stats && nr < 128) stats->results[nr] = result;
                ++nr;
                ok = result == 1;
            }
        }
        // the round's end: the level pass and the next round's vertex set, or the final pass and the write-back
        const bool last = round + 1 == opt.nrounds;
        if (!last) {
            // Optimizer.cc:1046-1049: the flag is read straight behind optimize(5); bDoMore = false skips the level pass too
            if (terminate()) { stopped = 2; break; }
            if (opt.classify) hipLaunchKernelGGL(k_ba_classify, g_pts, b_pt, 0, st, D, opt.chi2_mono, opt.chi2_stereo, 0);
            hipLaunchKernelGGL(k_ba_activate, dim3(1), dim3(RT), 0, st, D);
            ORBX_HIP(hipGetLastError());
            if (sc.download_head(round_head)) ORBX_FAIL(ORBX_ERR_HIP, "a round's read-back failed");
            nact = L.flag(LM_ISC_NACT);
            nactive_edges = L.flag(LM_ISC_NEDGES);
            if (env && nact > 0 && nactive_edges > 0) {                         // the next round's rows: its envelope, planned here, and the image the solver reads
                if ((rc = ba_env_plan(P, sc.r<int32_t>(o_ridx), nact, E)) != ORBX_OK) return rc;
                if ((size_t)E.live > tile_cap) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "the second round's envelope has more live tiles than the call reserved");
                const size_t bytes = (sizeof(int32_t) * E.image.size() + 15) & ~(size_t)15;
                memcpy(sc.w.pin + o_env, E.image.data(), sizeof(int32_t) * E.image.size());
                ORBX_HIP(orbx::stage_in(sc.w.dev + o_env, sc.w.pin + o_env, bytes, st));
                D.nt = E.nt;
            }
        }
    }
    if (opt.classify) hipLaunchKernelGGL(k_ba_classify, g_pts, b_pt, 0, st, D, opt.chi2_mono, opt.chi2_stereo, 1);
    hipLaunchKernelGGL(k_ba_final, g_all, b_pt, 0, st, D);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(out.poses, sc.r<float>(o_pout), sizeof(float) * 16 * nf);
    memcpy(out.points, sc.r<float>(o_xout), sizeof(float) * 3 * np);
    if (opt.classify) memcpy(out.erase, sc.r<uint8_t>(o_erase), ne);
    for (int n = 0; out.not_included && n < g.npoints; ++n) out.not_included[n] = (uint8_t)P.point_class[n];
    out.stopped = stopped ? stopped : (stop_seen ? 2 : 0);
    if (stats) {
        stats->rounds = rounds_run;
        for (int r = 0; r < 2; ++r) { stats->iterations[r] = st_iter[r]; stats->trials[r] = st_trials[r]; }
        stats->nresults = nr;
        stats->ntrials = L.nt; stats->trial_overflow = L.nt > stats->trial_capacity ? 1 : 0;
        if (stats->poses) memcpy(stats->poses, sc.r<double>(o_pd), sizeof(double) * 7 * nf);
        if (stats->points) memcpy(stats->points, sc.r<double>(o_xd), sizeof(double) * 3 * np);
        if (stats->chi2) memcpy(stats->chi2, sc.r<double>(o_chi), sizeof(double) * ne);
        if (stats->level) memcpy(stats->level, sc.r<uint8_t>(o_lout), ne);
    }
    g_last_ba_waits = sc.waits;
    return ORBX_OK;
}

} // namespace

int orbm_ba_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                 int32_t *block_start, int32_t *block_entries, int32_t *counts)
{
    return plan_out(g, BA_LOCAL, pose_class, point_class, pose_edge_start, pose_edges, block_start, block_entries, counts);
}

int orbm_global_ba_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                        int32_t *block_start, int32_t *block_entries, int32_t *counts)
{
    return plan_out(g, BA_GLOBAL, pose_class, point_class, pose_edge_start, pose_edges, block_start, block_entries, counts);
}

int orbm_global_ba_env_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                            int32_t *blk_i1, int32_t *blk_i2, int32_t *blk_start, int32_t *block_entries, int32_t *first, int32_t *counts)
{
    if (!g) ORBX_FAIL(ORBX_ERR_ARG, "null graph");
    BaPlan P;
    LltEnvPlan E;
    std::vector<int32_t> ridx0;
    int rc = ba_plan(*g, P, BA_ENV);
    if (rc == ORBX_OK) {
        const int nact0 = round0_rows(*g, P, ridx0);
        rc = ba_env_plan(P, ridx0.data(), nact0, E);
    }
    if (rc != ORBX_OK) return rc;
    auto copy = [](int32_t *dst, const std::vector<int32_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    copy(pose_class, P.pose_class); copy(point_class, P.point_class); copy(pose_edge_start, P.pe_start); copy(pose_edges, P.pe_list);
    copy(blk_i1, P.blk_i1); copy(blk_i2, P.blk_i2); copy(blk_start, P.blk_start); copy(block_entries, P.blk_ent); copy(first, E.first);
    if (counts) {
        counts[0] = (int32_t)P.pe_list.size(); counts[1] = (int32_t)(P.blk_ent.size() / 3); counts[2] = (int32_t)P.blk_i1.size();
        counts[3] = E.nt; counts[4] = E.live; counts[5] = E.launches;
    }
    return ORBX_OK;
}

int orbm_debug_last_ba_waits(void) { return g_last_ba_waits.load(); }

int orbm_bundle_adjustment(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag, orbm_ba_result *out,
                           orbm_ba_stats *stats)
{
    return ba_run(g, opt, stop_flag, out, stats, BA_LOCAL);
}

int orbm_global_bundle_adjustment(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag, orbm_ba_result *out,
                                  orbm_ba_stats *stats)
{
    return ba_run(g, opt, stop_flag, out, stats, BA_GLOBAL);
}

int orbm_global_bundle_adjustment_env(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag, orbm_ba_result *out,
                                      orbm_ba_stats *stats)
{
    return ba_run(g, opt, stop_flag, out, stats, BA_ENV);
}
