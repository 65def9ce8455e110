// orbm_essential_graph.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1165-1428) on the graph the caller has flattened
// (include/orbslam_hip.h).  The DECISIONS stay on the host, as in orbm_ba.hip: OptimizationAlgorithmLevenberg::solve
// (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:63-241, bInFEA false) with its trial loop, lambda and _ni, rho with
// + 1e-3, qmax, _nBad and Terminate, and SparseOptimizer::optimize's loop; computeLambdaInit returns the user's value (:245-246).
// The PASSES run on the device, and no workgroup ever waits for another:
//   k_eg_init        vScw of every vertex (its CorrectedSim3, else Sim3(R, t, 1.0) of the float pose, :1202-1216) = its first estimate;
//                    the measurement Sji of every edge in the formula order of :1241-1251 / :1273-1298
//   k_eg_errors      EdgeSim3::computeError (types/types_seven_dof_expmap.h:106-114) with Sim3::log (types/sim3.h:148-230), a thread
//                    per edge; the 7 doubles stored; chi2 per thread, wave, block
//   k_eg_linearize   BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205): a lane per (edge, side, dimension) runs
//                    oplus(+delta), error, oplus(-delta), error and scalar * (e+ - e-); the two 7 x 7 Jacobians go through LDS and the
//                    edge's 16 lanes form A^T A, A^T B, B^T B, -A^T e, -B^T e (constructQuadraticForm :55-90, omega = I), every dot in
//                    ascending k, into the edge's 161 doubles
//   k_eg_gather      a wave per vertex of the system: lane j sums entry j of its diagonal block (49) and of b (7) over its edges, in
//                    edge order
//   k_eg_assemble    S = H + lambda I: the WHOLE lower triangle of the column-major n x n square (the factorisation overwrites it),
//                    zeros, the diagonal blocks, every off-diagonal block summed over its pair's edges in edge order
//   orbm_llt_solve_dev   the solve (orbm_llt.hip), as it is, at every size
//   k_eg_assemble_env, orbm_llt_env_solve_dev   orbm_essential_graph_env: the same entries into the live tiles of the
//                    tile envelope the pair list gives, and the solve over those tiles; every other pass is shared
//   k_eg_update      push; x[6] = 0 in place when the scale is fixed (oplusImpl writes into the solver's vector); Sim3(x) * estimate;
//                    the terms of computeScale
//   k_eg_reduce      chi2's block partials in the fixed tree of orbm_ba.hip; computeScale's terms in index order by one thread
//   k_eg_pop, k_eg_final   the copies; [R | t / s] of every vertex (:1383-1393) and correctedSwr.map(Srw.map(P)) of every point (:1416-1423)
// No floating-point atomics and no matrix instruction: a call gives the same bytes from run to run.  The host waits once per trial
// (a 128-byte block: chi2 at the iteration's start, tempChi, scale, ok2) and once at the end.
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
#include "orbm_sim3_math.h"

using namespace orbm_detail;

namespace {

constexpr int PT = 64;                  // threads per block of the per-vertex / per-edge / per-point passes: one wave
constexpr int RT = 256;                 // the reduction's one block, and a block of k_eg_assemble
constexpr int EPW = 4;                  // edges per wave of k_eg_linearize: 16 lanes each, 14 of them own a Jacobian column
constexpr int NC = 161;                 // an edge's store: A^T A [49], A^T B [49], B^T B [49], -A^T e [7], -B^T e [7]
constexpr int EG_MAXACT = 438, EG_MAXVERT = 1024, EG_MAXEDGES = 32768, EG_MAXPOINTS = 1048576, EG_MAXITER = 64;
static_assert(7 * EG_MAXACT <= 3072 && 7 * (EG_MAXACT + 1) > 3072, "the system fits orbm_llt_solve_dev");
constexpr int EGE_MAXACT = 4096, EGE_MAXVERT = 8192, EGE_MAXEDGES = 131072;    // orbm_essential_graph_env
static_assert(7 * EGE_MAXACT == 28672, "the system fits orbm_llt_env_solve_dev");

// what the two entries differ in before the device is touched
struct EgLimits {
    int maxact, maxvert, maxedges;
    const char *act_msg, *vert_msg, *edges_msg;
};
constexpr EgLimits EG_DENSE = {EG_MAXACT, EG_MAXVERT, EG_MAXEDGES, "more than 438 free keyframes with an edge", "more than 1,024 keyframes",
                               "more than 32,768 edges"};
constexpr EgLimits EG_ENV = {EGE_MAXACT, EGE_MAXVERT, EGE_MAXEDGES, "more than 4,096 free keyframes with an edge", "more than 8,192 keyframes",
                             "more than 131,072 edges"};

// the call's arrays on the device
struct EgDev {
    int nvert, nedges, npoints, nact, n, fix_scale, nblocks;    // nblocks: blocks of k_eg_errors
    const float *poses_in, *points_in;
    const int *corrected, *noncorrected, *e_v0, *e_v1, *p_ref;
    const double *corr_tab, *nc_tab;
    const uint8_t *e_kind;
    const int *vclass, *act_vert, *ve_start, *ve_list, *col_start, *pair_hi, *pe_start, *pe_list;
    double *vscw, *est, *est_bak;       // [nvert][8]: q, t, s
    double *meas;                       // [nedges][8]
    double *e_err;                      // [nedges][7]: _error as the last computeError left it
    double *contrib;                    // [nedges][NC]
    double *Hd;                         // [nact][49]
    double *b, *x, *sterm;              // [n]
    double *S;                          // [n][n]
    double *A, *W;                      // the envelope entry: the live tiles and the solver's running dots in place of S
    const int *env;                     // its device plan image (orbm_llt_env.h)
    const int *tile_row;                // [live tiles]: the row tile of a packed tile
    int T, nt;                          // orbm_llt_tile(), ceil(n / T)
    double *part_chi;                   // [nblocks]
    double *sc;                         // the block a trial reads back (LM_SC_*, LM_ISC_*: orbm_internal.h)
    int *isc;
    float *poses_out, *points_out;
    double *est_out, *chi2_out;
};

__device__ __forceinline__ void load_sim3(const double *a, int k, Sim3 &S)
{
    const double *o = a + 8 * (size_t)k;
    S.q[0] = o[0]; S.q[1] = o[1]; S.q[2] = o[2]; S.q[3] = o[3]; S.t[0] = o[4]; S.t[1] = o[5]; S.t[2] = o[6]; S.s = o[7];
}
__device__ __forceinline__ void store_sim3(double *a, int k, const Sim3 &S)
{
    double *o = a + 8 * (size_t)k;
    o[0] = S.q[0]; o[1] = S.q[1]; o[2] = S.q[2]; o[3] = S.q[3]; o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = S.s;
}

// vScw[v] (:1202-1216)
__device__ __forceinline__ void vertex_scw(const EgDev &D, int v, Sim3 &S)
{
    const int c = D.corrected[v];
    if (c >= 0) { load_sim3(D.corr_tab, c, S); return; }
    const float *T = D.poses_in + 16 * (size_t)v;
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
    sim3_from_rts(R, t, 1.0f, S);
}

// Sim3::map
__device__ __forceinline__ void sim3_map(const Sim3 &S, const double X[3], double o[3])
{
    double r[3];
    q_rotate(S.q, X, r);
    ORBM_UNROLL for (int k = 0; k < 3; ++k) o[k] = S.s * r[k] + S.t[k];
}

// x = W^-1 t as Eigen's PartialPivLU of a fixed 3 x 3 runs it: the row of the largest |entry| of the column (the first one wins a
// tie) is swapped up, the column below divided by the pivot, the trailing block updated; then the permuted right-hand side through
// the unit lower and the upper triangle (a row's dot first, then the subtraction, then the division)
__device__ __forceinline__ void lu3_solve(double (&m)[9], const double t[3], double x[3])
{
#define W(i, j) m[3 * (i) + (j)]
    double y[3] = {t[0], t[1], t[2]};
    ORBM_UNROLL for (int k = 0; k < 3; ++k) {
        int p = k;
        double big = fabs(W(k, k));
        ORBM_UNROLL for (int i = k + 1; i < 3; ++i) {
            const double f = fabs(W(i, k));
            if (f > big) { big = f; p = i; }
        }
        ORBM_UNROLL for (int i = k + 1; i < 3; ++i)
            if (p == i) {
                ORBM_UNROLL for (int c = 0; c < 3; ++c) { const double s = W(k, c); W(k, c) = W(i, c); W(i, c) = s; }
                const double s = y[k]; y[k] = y[i]; y[i] = s;
            }
        if (big != 0.0)
            ORBM_UNROLL for (int i = k + 1; i < 3; ++i) W(i, k) /= W(k, k);
        ORBM_UNROLL for (int i = k + 1; i < 3; ++i)
            ORBM_UNROLL for (int c = k + 1; c < 3; ++c) W(i, c) -= W(i, k) * W(k, c);
    }
    y[1] -= W(1, 0) * y[0];
    y[2] -= W(2, 0) * y[0] + W(2, 1) * y[1];
    x[2] = y[2] / W(2, 2);
    x[1] = (y[1] - W(1, 2) * x[2]) / W(1, 1);
    x[0] = (y[0] - (W(0, 1) * x[1] + W(0, 2) * x[2])) / W(0, 0);
#undef W
}

// Sim3::log, types/sim3.h:148-230
__device__ __forceinline__ void sim3_log(const Sim3 &S, double res[7])
{
    const double s = S.s, sigma = log(s);
    double R[9];
    quat_to_matrix(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    double A, B, C, f;
    const bool near_identity = d > 1 - eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (near_identity) { f = 0.5; A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta = acos(d), theta2 = theta * theta;
            f = theta / (2 * sqrt(1 - d * d));
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (near_identity) {
            const double sigma2 = sigma * sigma;
            f = 0.5;
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            f = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta, a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double w0 = f * dR[0], w1 = f * dR[1], w2 = f * dR[2];
    const double Om[9] = {0., -w2, w1, w2, 0., -w0, -w1, w0, 0.};
    double BO[9], W[9];
    ORBM_UNROLL for (int k = 0; k < 9; ++k) BO[k] = B * Om[k];
    ORBM_UNROLL for (int i = 0; i < 3; ++i)
        ORBM_UNROLL for (int j = 0; j < 3; ++j) {
            const double o2 = BO[3 * i] * Om[j] + BO[3 * i + 1] * Om[3 + j] + BO[3 * i + 2] * Om[6 + j];
            W[3 * i + j] = A * Om[3 * i + j] + o2 + C * ((i == j) ? 1.0 : 0.0);
        }
    double u[3];
    lu3_solve(W, S.t, u);
    res[0] = w0; res[1] = w1; res[2] = w2; res[3] = u[0]; res[4] = u[1]; res[5] = u[2]; res[6] = sigma;
}

// EdgeSim3::computeError: (C * v1) * v2^-1, then log
__device__ __forceinline__ void edge_error(const Sim3 &Cm, const Sim3 &Si, const Sim3 &Sj, double e[7])
{
    Sim3 a, inv, err;
    sim3_mul(Cm, Si, a);
    sim3_inverse(Sj, inv);
    sim3_mul(a, inv, err);
    sim3_log(err, e);
}

__global__ __launch_bounds__(PT) void k_eg_init(EgDev D)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < D.nvert) {
        Sim3 S;
        vertex_scw(D, i, S);
        store_sim3(D.vscw, i, S);
        store_sim3(D.est, i, S);
        store_sim3(D.est_bak, i, S);
    }
    if (i < D.nedges) {
        const int vi = D.e_v0[i], vj = D.e_v1[i];
        Sim3 Siw, Sjw, Swi, Sji;
        if (D.e_kind[i] == 0) {                                     // :1241-1251
            vertex_scw(D, vi, Siw);
            sim3_inverse(Siw, Swi);
            vertex_scw(D, vj, Sjw);
        } else {                                                    // :1273-1298 (and :1316-1325, :1347-1356)
            if (D.noncorrected[vi] >= 0) load_sim3(D.nc_tab, D.noncorrected[vi], Siw);
            else vertex_scw(D, vi, Siw);
            sim3_inverse(Siw, Swi);
            if (D.noncorrected[vj] >= 0) load_sim3(D.nc_tab, D.noncorrected[vj], Sjw);
            else vertex_scw(D, vj, Sjw);
        }
        sim3_mul(Sjw, Swi, Sji);
        store_sim3(D.meas, i, Sji);
        for (int k = 0; k < 7; ++k) D.e_err[7 * (size_t)i + k] = 0.0;
    }
}

// _error . (information * _error), information = I
__device__ __forceinline__ double edge_chi2(const double e[7])
{
    double c = e[0] * e[0];
    ORBM_UNROLL for (int k = 1; k < 7; ++k) c = c + e[k] * e[k];
    return c;
}

// computeActiveErrors + activeRobustChi2 (no kernel on these edges)
__global__ __launch_bounds__(PT) void k_eg_errors(EgDev D)
{
    const int e = blockIdx.x * PT + threadIdx.x;
    double chi = 0.0;
    if (e < D.nedges) {
        Sim3 Cm, Si, Sj;
        load_sim3(D.meas, e, Cm);
        load_sim3(D.est, D.e_v0[e], Si);
        load_sim3(D.est, D.e_v1[e], Sj);
        double err[7];
        edge_error(Cm, Si, Sj, err);
        ORBM_UNROLL for (int k = 0; k < 7; ++k) D.e_err[7 * (size_t)e + k] = err[k];
        chi = edge_chi2(err);
    }
    chi = wave_sum(chi);
    if (threadIdx.x == 0) D.part_chi[blockIdx.x] = chi;
}

// linearizeOplus + constructQuadraticForm of EPW edges per wave
__global__ __launch_bounds__(PT) void k_eg_linearize(EgDev D)
{
    __shared__ double s_J[EPW][2][7][7];        // [edge][side][error row k][dimension d]
    __shared__ double s_e[EPW][7];
    const int slot = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int e = blockIdx.x * EPW + slot;
    const bool valid = e < D.nedges;
    int v0 = 0, v1 = 0;
    if (valid) { v0 = D.e_v0[e]; v1 = D.e_v1[e]; }
    if (valid && j < 14) {
        const int side = j >= 7 ? 1 : 0, d = j - 7 * side;
        double col[7];
        ORBM_UNROLL for (int k = 0; k < 7; ++k) col[k] = 0.0;
        if (D.vclass[side ? v1 : v0] != 1) {                        // a fixed side is skipped
            Sim3 Cm, Si, Sj;
            load_sim3(D.meas, e, Cm);
            load_sim3(D.est, v0, Si);
            load_sim3(D.est, v1, Sj);
            const double delta = 1e-9, scalar = 1.0 / (2 * delta);
#pragma unroll 1
            for (int sgn = 0; sgn < 2; ++sgn) {
                double u[7], err[7];
                const double step = sgn ? -delta : delta;
                ORBM_UNROLL for (int k = 0; k < 7; ++k) u[k] = (k == d) ? step : 0.0;
                if (D.fix_scale) u[6] = 0;                          // oplusImpl, also inside the numeric Jacobian
                Sim3 up, P;
                sim3_exp(u, up);
                sim3_mul(up, side ? Sj : Si, P);
                edge_error(Cm, side ? Si : P, side ? P : Sj, err);
                if (sgn == 0) { ORBM_UNROLL for (int k = 0; k < 7; ++k) col[k] = err[k]; }
                else { ORBM_UNROLL for (int k = 0; k < 7; ++k) col[k] = scalar * (col[k] - err[k]); }
            }
        }
        ORBM_UNROLL for (int k = 0; k < 7; ++k) s_J[slot][side][k][d] = col[k];
    }
    if (valid && j < 7) s_e[slot][j] = D.e_err[7 * (size_t)e + j];      // the stored error (errorBeforeNumeric)
    __syncthreads();
    if (!valid) return;
    double *out = D.contrib + NC * (size_t)e;
    for (int idx = j; idx < NC; idx += 16) {
        double v;
        if (idx < 147) {
            const int m = idx / 49, r = (idx % 49) / 7, c = idx % 7;
            const double (*X)[7] = s_J[slot][m == 2 ? 1 : 0], (*Y)[7] = s_J[slot][m == 0 ? 0 : 1];
            v = X[0][r] * Y[0][c];
            ORBM_UNROLL for (int k = 1; k < 7; ++k) v = v + X[k][r] * Y[k][c];
        } else {
            const int side = (idx - 147) / 7, r = (idx - 147) % 7;
            const double (*X)[7] = s_J[slot][side];
            v = X[0][r] * -s_e[slot][0];
            ORBM_UNROLL for (int k = 1; k < 7; ++k) v = v + X[k][r] * -s_e[slot][k];
        }
        out[idx] = v;
    }
}

// the diagonal block and b of the vertex of row blockIdx.x
__global__ __launch_bounds__(PT) void k_eg_gather(EgDev D)
{
    const int r = blockIdx.x, v = D.act_vert[r], l = threadIdx.x;
    if (l >= 56) return;
    double s = 0.0;
    for (int k = D.ve_start[v]; k < D.ve_start[v + 1]; ++k) {
        const int code = D.ve_list[k], e = code >> 1, side = code & 1;
        const int idx = l < 49 ? (side ? 98 : 0) + l : 147 + 7 * side + (l - 49);
        s += D.contrib[NC * (size_t)e + idx];
    }
    if (l < 49) D.Hd[49 * r + l] = s;
    else D.b[7 * r + (l - 49)] = s;
}

// Entry (row r of block row rb, column c of block column cb), rb >= cb, of S = H + lambda I as k_eg_assemble below forms it, value
// and summation order: the diagonal block plus lambda, or 0.0 + the pair's edges in edge order.  For k_eg_assemble_env, which has
// no block column of its own to hoist the pair range for; k_eg_assemble stays as it is.
__device__ __forceinline__ double system_entry(const EgDev &D, int rb, int r, int cb, int c, double lambda)
{
    double v = 0.0;
    if (rb == cb) {
        v = D.Hd[49 * cb + 7 * r + c];
        if (r == c) v += lambda;
        return v;
    }
    const int p1 = D.col_start[cb + 1];
    int lo = D.col_start[cb], hi = p1;                              // the pair (cb, rb), if an edge joins the two
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (D.pair_hi[mid] < rb) lo = mid + 1;
        else hi = mid;
    }
    if (lo < p1 && D.pair_hi[lo] == rb)
        for (int k = D.pe_start[lo]; k < D.pe_start[lo + 1]; ++k) {
            const int code = D.pe_list[k], e = code >> 1;
            // A^T B is (vertex 0) x (vertex 1): entry (row r of rb, column c of cb) is its transpose unless vertex 0 is rb
            v += D.contrib[NC * (size_t)e + 49 + ((code & 1) ? 7 * r + c : 7 * c + r)];
        }
    return v;
}

// S = H + lambda I, block column blockIdx.x: every entry on and below the diagonal; consecutive threads run down a column
__global__ __launch_bounds__(RT) void k_eg_assemble(EgDev D, double lambda)
{
    const int cb = blockIdx.x, n = D.n, r0 = 7 * cb, nrows = n - r0;
    const int p0 = D.col_start[cb], p1 = D.col_start[cb + 1];
    for (int idx = threadIdx.x; idx < 7 * nrows; idx += RT) {
        const int c = idx / nrows, row = r0 + idx % nrows, col = r0 + c;
        if (row < col) continue;
        const int rb = row / 7, r = row - 7 * rb;
        double v = 0.0;
        if (rb == cb) {
            v = D.Hd[49 * cb + 7 * r + c];
            if (r == c) v += lambda;
        } else {
            int lo = p0, hi = p1;                                   // the pair (cb, rb), if an edge joins the two
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (D.pair_hi[mid] < rb) lo = mid + 1;
                else hi = mid;
            }
            if (lo < p1 && D.pair_hi[lo] == rb)
                for (int k = D.pe_start[lo]; k < D.pe_start[lo + 1]; ++k) {
                    const int code = D.pe_list[k], e = code >> 1;
                    // A^T B is (vertex 0) x (vertex 1): entry (row r of rb, column c of cb) is its transpose unless vertex 0 is rb
                    v += D.contrib[NC * (size_t)e + 49 + ((code & 1) ? 7 * r + c : 7 * c + r)];
                }
        }
        D.S[(size_t)col * n + row] = v;
    }
}

// The same entries into live tile blockIdx.x of the envelope (orbm_llt_env_solve_dev's packing): EVERY entry on and below the
// diagonal with a row below n, the zeros too (the factorisation has overwritten the tile with fill-in)
__global__ __launch_bounds__(RT) void k_eg_assemble_env(EgDev D, double lambda)
{
    const int T = D.T, t = blockIdx.x, R = D.tile_row[t];
    const int C = LltEnvView(D.env, D.nt).col_of(R, t);
    double *tile = D.A + (size_t)t * T * T;
    for (int idx = threadIdx.x; idx < T * T; idx += RT) {
        const int row = R * T + idx % T, col = C * T + idx / T;
        if (row >= D.n || row < col) continue;
        const int rb = row / 7, cb = col / 7;
        tile[idx] = system_entry(D, rb, row - 7 * rb, cb, col - 7 * cb, lambda);
    }
}

// push; oplus; the vertex's terms of computeScale.  A thread per vertex of the system.
__global__ __launch_bounds__(PT) void k_eg_update(EgDev D, double lambda)
{
    const int r = blockIdx.x * PT + threadIdx.x;
    if (r >= D.nact) return;
    const int v = D.act_vert[r];
    Sim3 T;
    load_sim3(D.est, v, T);
    store_sim3(D.est_bak, v, T);
    double x[7];
    ORBM_UNROLL for (int j = 0; j < 7; ++j) x[j] = D.x[7 * r + j];
    if (D.fix_scale) { x[6] = 0; D.x[7 * r + 6] = 0; }
    const bool ok = D.isc[LM_ISC_OK2] != 0;
    if (ok) {
        Sim3 up, o;
        sim3_exp(x, up);
        sim3_mul(up, T, o);
        store_sim3(D.est, v, o);
    }
    ORBM_UNROLL for (int j = 0; j < 7; ++j) D.sterm[7 * r + j] = ok ? x[j] * (lambda * x[j] + D.b[7 * r + j]) : 0.0;
}

__global__ __launch_bounds__(PT) void k_eg_pop(EgDev D)
{
    const int r = blockIdx.x * PT + threadIdx.x;
    if (r >= D.nact) return;
    const int v = D.act_vert[r];
    for (int j = 0; j < 8; ++j) D.est[8 * (size_t)v + j] = D.est_bak[8 * (size_t)v + j];
}

// mode 0: chi2 at the iteration's start.  mode 1: tempChi, and computeScale over the solver's vector in index order.  One block.
__global__ __launch_bounds__(RT) void k_eg_reduce(EgDev D, int mode)
{
    __shared__ double s_red[RT / 64][1];
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < D.nblocks; b += RT) v[0] += D.part_chi[b];
    block_sum<1, RT / 64>(v, s_red);
    if (threadIdx.x == 0) {
        if (!mode) D.sc[LM_SC_CHI2] = v[0];
        else {
            double s = 0.0;
            for (int i = 0; i < D.n; ++i) s += D.sterm[i];
            D.sc[LM_SC_TEMPCHI] = v[0]; D.sc[LM_SC_SCALE] = s;
        }
    }
}

// write-back: a vertex's [R | t / s]; a point through Srw and the inverse of its reference's final estimate
__global__ __launch_bounds__(PT) void k_eg_final(EgDev D)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < D.nvert) {
        Sim3 S;
        load_sim3(D.est, i, S);
        double R[9];
        quat_to_matrix(S.q, R);
        const double f = 1. / S.s;
        float *o = D.poses_out + 16 * (size_t)i;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)R[3 * r + c];
            o[4 * r + 3] = (float)(S.t[r] * f);
        }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
        for (int j = 0; j < 8; ++j) D.est_out[8 * (size_t)i + j] = D.est[8 * (size_t)i + j];
    }
    if (i < D.npoints) {
        const int ref = D.p_ref[i];
        Sim3 Srw, Siw, Swr;
        load_sim3(D.vscw, ref, Srw);
        load_sim3(D.est, ref, Siw);
        sim3_inverse(Siw, Swr);                                     // vCorrectedSwc[nIDr]
        const double P[3] = {(double)D.points_in[3 * (size_t)i], (double)D.points_in[3 * (size_t)i + 1], (double)D.points_in[3 * (size_t)i + 2]};
        double a[3], c[3];
        sim3_map(Srw, P, a);
        sim3_map(Swr, a, c);
        for (int j = 0; j < 3; ++j) D.points_out[3 * (size_t)i + j] = (float)c[j];
    }
    if (i < D.nedges) {
        double err[7];
        for (int k = 0; k < 7; ++k) err[k] = D.e_err[7 * (size_t)i + k];
        D.chi2_out[i] = edge_chi2(err);
    }
}

// ---- host

struct EgPlan {
    int nact = 0;
    std::vector<int32_t> vclass, row, act_vert, ve_start, ve_list, col_start, pair_start, pair_v, pair_hi, pe_list;
};

// arguments, limits, indices; the vertex classes, the vertex -> edge lists and the pair -> edge lists
int eg_plan(const orbm_eg_graph &g, EgPlan &P, const EgLimits &lim)
{
    if (g.nvert < 0 || g.ncorr < 0 || g.nnc < 0 || g.nedges < 0 || g.npoints < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative size");
    if (g.nvert > lim.maxvert) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, lim.vert_msg);
    if (g.nedges > lim.maxedges) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, lim.edges_msg);
    if (g.npoints > EG_MAXPOINTS) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,048,576 points");
    if ((g.nvert && (!g.poses || !g.corrected || !g.noncorrected || !g.fixed)) || (g.ncorr && !g.corrected_sim3) || (g.nnc && !g.noncorrected_sim3) ||
        (g.nedges && (!g.e_v0 || !g.e_v1 || !g.e_kind)) || (g.npoints && (!g.points || !g.p_ref)))
        ORBX_FAIL(ORBX_ERR_ARG, "null pointer in the graph");
    const int nv = g.nvert;
    P.vclass.assign((size_t)nv, 2);
    for (int v = 0; v < nv; ++v) {
        if (g.corrected[v] < -1 || g.corrected[v] >= g.ncorr) ORBX_FAIL(ORBX_ERR_ARG, "a CorrectedSim3 index is out of range");
        if (g.noncorrected[v] < -1 || g.noncorrected[v] >= g.nnc) ORBX_FAIL(ORBX_ERR_ARG, "a NonCorrectedSim3 index is out of range");
        if (g.fixed[v]) P.vclass[v] = 1;
    }
    for (int e = 0; e < g.nedges; ++e) {
        const int a = g.e_v0[e], b = g.e_v1[e];
        if (a < 0 || a >= nv || b < 0 || b >= nv) ORBX_FAIL(ORBX_ERR_ARG, "an edge's vertex index is out of range");
        if (a == b) ORBX_FAIL(ORBX_ERR_ARG, "an edge joins a vertex with itself");
        if (g.e_kind[e] > 1) ORBX_FAIL(ORBX_ERR_ARG, "an edge's kind is 0 or 1");
        if (g.fixed[a] && g.fixed[b]) ORBX_FAIL(ORBX_ERR_ARG, "an edge joins two fixed vertices");
        if (P.vclass[a] == 2) P.vclass[a] = 0;
        if (P.vclass[b] == 2) P.vclass[b] = 0;
    }
    for (int i = 0; i < g.npoints; ++i)
        if (g.p_ref[i] < 0 || g.p_ref[i] >= nv) ORBX_FAIL(ORBX_ERR_ARG, "a point's reference index is out of range");
    P.row.assign((size_t)nv, -1);
    P.act_vert.clear();
    for (int v = 0; v < nv; ++v)
        if (P.vclass[v] == 0) { P.row[v] = (int32_t)P.act_vert.size(); P.act_vert.push_back(v); }
    P.nact = (int)P.act_vert.size();
    if (P.nact > lim.maxact) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, lim.act_msg);
    auto finite = [](const auto *a, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite((double)a[i])) return false; return true; };
    if (!finite(g.poses, 16 * (size_t)nv) || !finite(g.corrected_sim3, 8 * (size_t)g.ncorr) || !finite(g.noncorrected_sim3, 8 * (size_t)g.nnc) ||
        !finite(g.points, 3 * (size_t)g.npoints))
        ORBX_FAIL(ORBX_ERR_ARG, "a non-finite input value");
    // vertex -> edges
    P.ve_start.assign((size_t)nv + 1, 0);
    for (int e = 0; e < g.nedges; ++e) {
        if (P.vclass[g.e_v0[e]] == 0) P.ve_start[(size_t)g.e_v0[e] + 1]++;
        if (P.vclass[g.e_v1[e]] == 0) P.ve_start[(size_t)g.e_v1[e] + 1]++;
    }
    for (int v = 0; v < nv; ++v) P.ve_start[(size_t)v + 1] += P.ve_start[v];
    P.ve_list.assign((size_t)P.ve_start[nv], 0);
    {
        std::vector<int32_t> fill(P.ve_start.begin(), P.ve_start.end() - 1);
        for (int e = 0; e < g.nedges; ++e) {
            if (P.vclass[g.e_v0[e]] == 0) P.ve_list[(size_t)fill[g.e_v0[e]]++] = 2 * e;
            if (P.vclass[g.e_v1[e]] == 0) P.ve_list[(size_t)fill[g.e_v1[e]]++] = 2 * e + 1;
        }
    }
    // pair -> edges: (smaller row, larger row, edge) sorted; the edge index keeps a pair's edges in edge order
    struct Ent { int32_t lo, hi, code; };
    std::vector<Ent> ents;
    for (int e = 0; e < g.nedges; ++e) {
        const int ra = P.row[g.e_v0[e]], rb = P.row[g.e_v1[e]];
        if (ra < 0 || rb < 0) continue;
        ents.push_back(ra < rb ? Ent{ra, rb, 2 * e} : Ent{rb, ra, 2 * e + 1});
    }
    std::sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) {
        if (a.lo != b.lo) return a.lo < b.lo;
        if (a.hi != b.hi) return a.hi < b.hi;
        return a.code < b.code;
    });
    P.col_start.assign((size_t)P.nact + 1, 0);
    P.pair_start.assign(1, 0);
    P.pair_v.clear(); P.pair_hi.clear(); P.pe_list.clear();
    for (size_t k = 0; k < ents.size(); ++k) {
        if (k == 0 || ents[k].lo != ents[k - 1].lo || ents[k].hi != ents[k - 1].hi) {
            if (k) P.pair_start.push_back((int32_t)k);
            P.pair_v.push_back(P.act_vert[ents[k].lo]); P.pair_v.push_back(P.act_vert[ents[k].hi]);
            P.pair_hi.push_back(ents[k].hi);
            P.col_start[(size_t)ents[k].lo + 1]++;
        }
        P.pe_list.push_back(ents[k].code);
    }
    if (!ents.empty()) P.pair_start.push_back((int32_t)ents.size());
    for (int r = 0; r < P.nact; ++r) P.col_start[(size_t)r + 1] += P.col_start[r];
    return ORBX_OK;
}

// The tile envelope of the system in the caller's vertex order, and what orbm_llt_env_solve_dev reads on the device: first[R] = the
// smallest column tile over the pairs (and the diagonal blocks) of the block rows that reach into row tile R.  tile_row[t]: the row
// tile of live tile t.  Refuses as orbm_llt_env_plan does (more than 8,192 live tiles).
struct EgEnvPlan : LltEnvPlan {
    std::vector<int32_t> tile_row;
};

int eg_env_plan(const EgPlan &P, EgEnvPlan &E)
{
    const int T = orbm_llt_tile();
    E.tile_row.clear();
    llt_env_start(E, 7 * P.nact);
    for (int r = 0; r < P.nact; ++r) {                              // block (rb, r), rb >= r: rows 7 rb .. 7 rb + 6, columns from 7 r
        llt_env_reach(E.first, T, 7 * r, 7 * r + 6, 7 * r);
        for (int k = P.col_start[(size_t)r]; k < P.col_start[(size_t)r + 1]; ++k) llt_env_reach(E.first, T, 7 * P.pair_hi[(size_t)k], 7 * P.pair_hi[(size_t)k] + 6, 7 * r);
    }
    if (const int e = llt_env_finish(E)) return e;
    for (int R = 0; R < E.nt; ++R) E.tile_row.insert(E.tile_row.end(), (size_t)(R - E.first[(size_t)R] + 1), R);     // off[R + 1] - off[R] tiles
    return ORBX_OK;
}

std::atomic<int> g_last_eg_waits{0};    // host waits of the last orbm_essential_graph of this process

void reset_stats(orbm_eg_stats *st)
{
    if (!st) return;
    st->iterations = 0; st->trials = 0; st->nresults = 0;
    for (int j = 0; j < 64; ++j) st->results[j] = 0;
    st->ntrials = 0; st->trial_overflow = 0;
}

} // namespace

int orbm_eg_plan(const orbm_eg_graph *g, int32_t *vertex_class, int32_t *row, int32_t *vert_edge_start, int32_t *vert_edges,
                 int32_t *pair_start, int32_t *pair_v, int32_t *pair_edges, int32_t *counts)
{
    if (!g) ORBX_FAIL(ORBX_ERR_ARG, "null graph");
    EgPlan P;
    const int rc = eg_plan(*g, P, EG_DENSE);
    if (rc != ORBX_OK) return rc;
    auto copy = [](int32_t *dst, const std::vector<int32_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    copy(vertex_class, P.vclass); copy(row, P.row); copy(vert_edge_start, P.ve_start); copy(vert_edges, P.ve_list);
    copy(pair_start, P.pair_start); copy(pair_v, P.pair_v); copy(pair_edges, P.pe_list);
    if (counts) { counts[0] = (int32_t)P.ve_list.size(); counts[1] = (int32_t)P.pair_hi.size(); counts[2] = (int32_t)P.pe_list.size(); }
    return ORBX_OK;
}

int orbm_eg_env_plan(const orbm_eg_graph *g, int32_t *vertex_class, int32_t *row, int32_t *vert_edge_start, int32_t *vert_edges,
                     int32_t *pair_start, int32_t *pair_v, int32_t *pair_edges, int32_t *first, int32_t *counts)
{
    if (!g) ORBX_FAIL(ORBX_ERR_ARG, "null graph");
    EgPlan P;
    EgEnvPlan E;
    int rc = eg_plan(*g, P, EG_ENV);
    if (rc == ORBX_OK) rc = eg_env_plan(P, E);
    if (rc != ORBX_OK) return rc;
    auto copy = [](int32_t *dst, const std::vector<int32_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    copy(vertex_class, P.vclass); copy(row, P.row); copy(vert_edge_start, P.ve_start); copy(vert_edges, P.ve_list);
    copy(pair_start, P.pair_start); copy(pair_v, P.pair_v); copy(pair_edges, P.pe_list); copy(first, E.first);
    if (counts) {
        counts[0] = (int32_t)P.ve_list.size(); counts[1] = (int32_t)P.pair_hi.size(); counts[2] = (int32_t)P.pe_list.size();
        counts[3] = E.nt; counts[4] = E.live; counts[5] = E.launches;
    }
    return ORBX_OK;
}

int orbm_debug_last_eg_waits(void) { return g_last_eg_waits.load(); }

namespace {

// The body of both public entries.  env: the limits of orbm_essential_graph_env, its assembly into the live tiles of the envelope and
// the solve over them; everything else is one code.
int eg_run(const orbm_eg_graph *gp, const orbm_eg_options *op, orbm_eg_result *outp, orbm_eg_stats *stats, bool env)
{
    if (!gp || !op || !outp) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    const orbm_eg_graph &g = *gp;
    const orbm_eg_options &opt = *op;
    orbm_eg_result &out = *outp;
    EgPlan P;
    EgEnvPlan E;
    int rc = eg_plan(g, P, env ? EG_ENV : EG_DENSE);
    if (rc != ORBX_OK) return rc;
    if (opt.iterations < 0 || opt.iterations > EG_MAXITER) ORBX_FAIL(ORBX_ERR_ARG, "iterations outside 0 .. 64");
    if (!(opt.lambda_init > 0) || !std::isfinite(opt.lambda_init)) ORBX_FAIL(ORBX_ERR_ARG, "lambda_init must be positive and finite");
    if ((g.nvert && !out.poses) || (g.npoints && !out.points)) ORBX_FAIL(ORBX_ERR_ARG, "null result array");
    if (stats && stats->trial_capacity < 0) ORBX_FAIL(ORBX_ERR_ARG, "negative trial capacity");
    if (stats && stats->trial_capacity > 0 && !stats->trial_log) ORBX_FAIL(ORBX_ERR_ARG, "trial capacity without a trial log");
    if (env && (rc = eg_env_plan(P, E)) != ORBX_OK) return rc;                  // the tile cap, behind every argument check (also when no solve will run)
    g_last_eg_waits = 0;
    reset_stats(stats);
    if (g.nvert == 0) return ORBX_OK;                                           // (no vertex: no edge and no point either)
    ORBX_NEED_DEVICE();

    // (with its initialiser, as orbm_ba.hip's: the lease-site table of tests/workspace_cases.py lists the calls whose stale-arena case
    // lives there; this call's case is tests/test_gpu_essential_graph_workspace.py)
    StagedCall sc{};
    EgDev D;
    memset(&D, 0, sizeof(D));
    const size_t nv = (size_t)g.nvert, ne = (size_t)g.nedges, np = (size_t)g.npoints, na = (size_t)P.nact, n = 7 * na;
    const size_t nblk = (ne + PT - 1) / PT, npairs = P.pair_hi.size();
    const bool solve = g.nedges > 0 && P.nact > 0 && opt.iterations > 0;
    D.nvert = g.nvert; D.nedges = g.nedges; D.npoints = g.npoints; D.nact = P.nact; D.n = (int)n; D.fix_scale = g.fix_scale ? 1 : 0; D.nblocks = (int)nblk;
    const size_t o_poses = sc.in(g.poses, sizeof(float) * 16 * nv), o_points = sc.in(g.points, sizeof(float) * 3 * np);
    const size_t o_cor = sc.in(g.corrected, sizeof(int32_t) * nv), o_nc = sc.in(g.noncorrected, sizeof(int32_t) * nv);
    const size_t o_ctab = sc.in(g.corrected_sim3, sizeof(double) * 8 * (size_t)g.ncorr), o_ntab = sc.in(g.noncorrected_sim3, sizeof(double) * 8 * (size_t)g.nnc);
    const size_t o_v0 = sc.in(g.e_v0, sizeof(int32_t) * ne), o_v1 = sc.in(g.e_v1, sizeof(int32_t) * ne), o_kind = sc.in(g.e_kind, ne);
    const size_t o_ref = sc.in(g.p_ref, sizeof(int32_t) * np);
    const size_t o_vc = sc.in(P.vclass.data(), sizeof(int32_t) * nv);
    const size_t o_av = sc.in(P.act_vert.data(), sizeof(int32_t) * na), o_vs = sc.in(P.ve_start.data(), sizeof(int32_t) * (nv + 1));
    const size_t o_vl = sc.in(P.ve_list.data(), sizeof(int32_t) * P.ve_list.size()), o_cs = sc.in(P.col_start.data(), sizeof(int32_t) * (na + 1));
    const size_t o_ph = sc.in(P.pair_hi.data(), sizeof(int32_t) * npairs), o_ps = sc.in(P.pair_start.data(), sizeof(int32_t) * P.pair_start.size());
    const size_t o_pl = sc.in(P.pe_list.data(), sizeof(int32_t) * P.pe_list.size());
    const size_t o_env = sc.in(E.image.data(), sizeof(int32_t) * E.image.size()), o_tr = sc.in(E.tile_row.data(), sizeof(int32_t) * E.tile_row.size());
    const size_t o_vscw = sc.scratch(sizeof(double) * 8 * nv), o_est = sc.scratch(sizeof(double) * 8 * nv), o_estb = sc.scratch(sizeof(double) * 8 * nv);
    const size_t o_meas = sc.scratch(sizeof(double) * 8 * ne), o_err = sc.scratch(sizeof(double) * 7 * ne);
    const size_t o_cb = sc.scratch(solve ? sizeof(double) * NC * ne : 0), o_Hd = sc.scratch(sizeof(double) * 49 * na);
    const size_t o_b = sc.scratch(sizeof(double) * n), o_x = sc.scratch(sizeof(double) * n), o_st = sc.scratch(sizeof(double) * n);
    const size_t tile_bytes = sizeof(double) * (size_t)E.live * (size_t)orbm_llt_tile() * (size_t)orbm_llt_tile();
    const size_t o_S = sc.scratch(solve && !env ? sizeof(double) * n * n : 0), o_pchi = sc.scratch(sizeof(double) * nblk);
    const size_t o_A = sc.scratch(solve && env ? tile_bytes : 0), o_W = sc.scratch(solve && env ? tile_bytes : 0);
    const size_t o_sc = sc.out(LM_BLOCK_BYTES);                                 // what a trial reads back
    const size_t o_pout = sc.out(sizeof(float) * 16 * nv), o_xout = sc.out(sizeof(float) * 3 * np);
    const size_t o_eout = sc.out(sizeof(double) * 8 * nv), o_chi = sc.out(sizeof(double) * ne);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    D.poses_in = sc.d<float>(o_poses); D.points_in = sc.d<float>(o_points); D.corrected = sc.d<int>(o_cor); D.noncorrected = sc.d<int>(o_nc);
    D.corr_tab = sc.d<double>(o_ctab); D.nc_tab = sc.d<double>(o_ntab); D.e_v0 = sc.d<int>(o_v0); D.e_v1 = sc.d<int>(o_v1);
    D.e_kind = sc.d<uint8_t>(o_kind); D.p_ref = sc.d<int>(o_ref); D.vclass = sc.d<int>(o_vc);
    D.act_vert = sc.d<int>(o_av); D.ve_start = sc.d<int>(o_vs); D.ve_list = sc.d<int>(o_vl); D.col_start = sc.d<int>(o_cs);
    D.pair_hi = sc.d<int>(o_ph); D.pe_start = sc.d<int>(o_ps); D.pe_list = sc.d<int>(o_pl);
    D.vscw = sc.d<double>(o_vscw); D.est = sc.d<double>(o_est); D.est_bak = sc.d<double>(o_estb); D.meas = sc.d<double>(o_meas);
    D.e_err = sc.d<double>(o_err); D.contrib = sc.d<double>(o_cb); D.Hd = sc.d<double>(o_Hd); D.b = sc.d<double>(o_b); D.x = sc.d<double>(o_x);
    D.sterm = sc.d<double>(o_st); D.S = sc.d<double>(o_S); D.part_chi = sc.d<double>(o_pchi);
    D.A = sc.d<double>(o_A); D.W = sc.d<double>(o_W); D.env = sc.d<int>(o_env); D.tile_row = sc.d<int>(o_tr); D.T = orbm_llt_tile(); D.nt = E.nt;
    D.sc = sc.d<double>(o_sc); D.isc = reinterpret_cast<int *>(sc.d<double>(o_sc) + 8);
    D.poses_out = sc.d<float>(o_pout); D.points_out = sc.d<float>(o_xout); D.est_out = sc.d<double>(o_eout); D.chi2_out = sc.d<double>(o_chi);

    hipStream_t st = sc.stream();
    const size_t nall = std::max(std::max(nv, np), ne);
    const dim3 g_all((unsigned)((nall + PT - 1) / PT)), g_init((unsigned)((std::max(nv, ne) + PT - 1) / PT)), g_edges((unsigned)nblk), b_pt(PT);
    const dim3 g_act((unsigned)((na + PT - 1) / PT)), g_lin((unsigned)((ne + EPW - 1) / EPW));
    LmHostLoop L{sc, stats ? stats->trial_log : nullptr, stats ? stats->trial_capacity : 0};

    hipLaunchKernelGGL(k_eg_init, g_init, b_pt, 0, st, D);
    int nr = 0, n_iter = 0, n_trials = 0;
    if (solve) {
        bool ok = true;
        for (int it = 0; it < opt.iterations && ok; ++it) {                     // SparseOptimizer::optimize
            hipLaunchKernelGGL(k_eg_errors, g_edges, b_pt, 0, st, D);
            hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(RT), 0, st, D, 0);
            hipLaunchKernelGGL(k_eg_linearize, g_lin, b_pt, 0, st, D);
            hipLaunchKernelGGL(k_eg_gather, dim3((unsigned)na), b_pt, 0, st, D);
            if (it == 0) L.lm.start(opt.lambda_init);                           // levenberg.cpp:110-115, computeLambdaInit :245-246
            auto trial = [&](double lambda) -> int {
                if (env) {
                    hipLaunchKernelGGL(k_eg_assemble_env, dim3((unsigned)E.live), dim3(RT), 0, st, D, lambda);
                    if (const int e = orbm_llt_env_solve_dev((int)n, E.first.data(), D.env, D.A, D.W, D.b, D.x, D.isc + LM_ISC_OK2, st)) return e;
                } else {
                    hipLaunchKernelGGL(k_eg_assemble, dim3((unsigned)na), dim3(RT), 0, st, D, lambda);
                    if (const int e = orbm_llt_solve_dev((int)n, D.S, D.b, D.x, D.isc + LM_ISC_OK2, st)) return e;
                }
                hipLaunchKernelGGL(k_eg_update, g_act, b_pt, 0, st, D, lambda);
                hipLaunchKernelGGL(k_eg_errors, g_edges, b_pt, 0, st, D);
                hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(RT), 0, st, D, 1);
                return ORBX_OK;
            };
            auto after_read = [&]() { if (L.qmax == 0) L.currentChi = L.iniChi = L.scalar(LM_SC_CHI2); };      // levenberg.cpp:97-99
            auto pop = [&]() { hipLaunchKernelGGL(k_eg_pop, g_act, b_pt, 0, st, D); };
            if ((rc = L.trials(0, trial, after_read, pop)) != ORBX_OK) return rc;
            ++n_iter;
            n_trials += L.qmax;
            const int result = L.lm.end_iteration(L.qmax, L.rho, L.iniChi, L.currentChi);
            if (stats && nr < 64) stats->results[nr] = result;
            ++nr;
            ok = result == 1;
        }
    }
    hipLaunchKernelGGL(k_eg_final, g_all, b_pt, 0, st, D);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(out.poses, sc.r<float>(o_pout), sizeof(float) * 16 * nv);
    if (np) memcpy(out.points, sc.r<float>(o_xout), sizeof(float) * 3 * np);
    if (stats) {
        stats->iterations = n_iter; stats->trials = n_trials; stats->nresults = nr;
        stats->ntrials = L.nt; stats->trial_overflow = L.nt > stats->trial_capacity ? 1 : 0;
        if (stats->estimates) memcpy(stats->estimates, sc.r<double>(o_eout), sizeof(double) * 8 * nv);
        if (stats->chi2 && ne) memcpy(stats->chi2, sc.r<double>(o_chi), sizeof(double) * ne);
    }
    g_last_eg_waits = sc.waits;
    return ORBX_OK;
}

} // namespace

int orbm_essential_graph(const orbm_eg_graph *g, const orbm_eg_options *opt, orbm_eg_result *out, orbm_eg_stats *stats)
{
    return eg_run(g, opt, out, stats, false);
}

int orbm_essential_graph_env(const orbm_eg_graph *g, const orbm_eg_options *opt, orbm_eg_result *out, orbm_eg_stats *stats)
{
    return eg_run(g, opt, out, stats, true);
}
