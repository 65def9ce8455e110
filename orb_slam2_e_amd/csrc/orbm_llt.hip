// orbm_llt.hip -- dense Cholesky solve of a system wider than one workgroup can factorise (include/orbslam_hip.h,
// orbm_llt_solve_dev).  S = L L^T in place on the lower triangle, L y = b, L^T x = y, in T x T tiles over many
// workgroups, and every number by the operations of k_ba_solve (orbm_ba.hip) in k_ba_solve's order:
//   L[i][j] = (a[i][j] - dot) / L[j][j],  dot = L[i][0] L[j][0], then dot = dot + L[i][k] L[j][k] for k = 1 .. j - 1 ascending
// The order is per ENTRY, so a tiled, right-looking factorisation keeps it: every lower entry (i, j) that is not final yet owns ONE
// running dot, held at the mirrored place S[i * n + j] of the strict upper triangle (the diagonal's in x, which is free until the
// substitutions); when panel K's columns are final every trailing entry adds the panel's T products in ascending k.
//   k_llt_diag0    the first diagonal tile, one workgroup
//   k_llt_rows     panel K: a workgroup per row tile below the diagonal tile solves its rows against the FINAL diagonal tile
//   k_llt_update   panel K: a workgroup per trailing tile adds the panel's products to its running dots; the workgroup of the NEXT
//                  diagonal tile then holds that tile's complete dots and factorises it on the spot
//   k_llt_fwd / k_llt_bwd   the substitutions, a launch per panel: every row tile subtracts the panel's T final unknowns in order;
//                  the tile that is complete with that divides through its own diagonal tile
// A diagonal tile is written by ONE workgroup, in a launch in which no other workgroup reads it (the launch BEFORE the one whose
// workgroups solve against it): no workgroup waits for another, ordering is the stream's, every loop is bounded by n or T.  4 nt - 1
// launches for nt = ceil(n / T) tiles.  A pivot that is not > 0 clears *ok; every later launch reads it first and does nothing,
// the substitutions write x = 0 instead.  Plain double multiplies and adds (-ffp-contract=off), no MFMA, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../../include/orbslam_hip.h"
#include "common.h"

namespace {

constexpr int T = 64;                   // tile edge
constexpr int NT = 256;                 // threads per workgroup; thread t < T owns row (or column) t of the tile in the serial parts
constexpr int LD = T + 1;               // row stride of a tile in LDS: rows read by lanes fall on distinct banks
constexpr int KH = 32;                  // the update's strips go through LDS in two halves of the panel
constexpr int LLT_MAXN = 3072;
// the k loops of the serial parts: the two LDS reads of a step do not depend on the running sum, so eight steps' reads are issued
// together and only the adds stay a chain (the order of the adds is the source's: nothing is reassociated)
#define LLT_UNROLL_K _Pragma("unroll 8")
static_assert(T % KH == 0 && NT == (T / 4) * (T / 4), "4 x 4 entries per thread");

struct Llt {
    int n, nt;
    double *S;
    const double *b;
    double *x;
    int *ok;
};

// the flag: one workgroup may clear it while others of the same launch read it (either value makes them do what they should: the
// launch's results are not used once it is 0), so both sides are relaxed atomics and not plain accesses
__device__ __forceinline__ int flag_read(int *ok) { return __hip_atomic_load(ok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void flag_write(int *ok, int v) { __hip_atomic_store(ok, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int tile_rows(const Llt &P, int R) { const int r = P.n - R * T; return r < T ? r : T; }

// D[x][y] (x >= y) = entry (c0 + x, c0 + y) of the lower triangle, all threads; the upper part of D is left alone
__device__ __forceinline__ void load_diag_lower(const Llt &P, int c0, int tw, double *D)
{
    for (int idx = threadIdx.x; idx < T * T; idx += NT) {
        const int x = idx % T, y = idx / T;
        if (x >= y && x < tw) D[x * LD + y] = P.S[(size_t)(c0 + y) * P.n + c0 + x];
    }
}

// The diagonal tile at c0, tw wide, in D: the lower part holds a, and with has_dots D[j][r] (r > j) the running dot of entry (r, j)
// and dd[r] the diagonal's.  Thread t owns row t.  Leaves L in the lower part of D and writes it to S; 0 (in every thread) at a
// pivot that is not > 0, with nothing written.
__device__ int factor_diag(const Llt &P, int c0, int tw, double *D, const double *dd, bool has_dots, int *s_fail, double *s_piv)
{
    const int t = threadIdx.x;
    if (t == 0) *s_fail = 0;
    __syncthreads();
    for (int j = 0; j < tw; ++j) {
        double s = 0.0;
        if (t >= j && t < tw) {
            s = D[t * LD + j];
            if (has_dots) {
                double dot = t == j ? dd[t] : D[j * LD + t];
                LLT_UNROLL_K
                for (int k = 0; k < j; ++k) dot = dot + D[t * LD + k] * D[j * LD + k];
                s = s - dot;
            } else if (j > 0) {
                double dot = D[t * LD] * D[j * LD];
                LLT_UNROLL_K
                for (int k = 1; k < j; ++k) dot = dot + D[t * LD + k] * D[j * LD + k];
                s = s - dot;
            }
        }
        if (t == j) {
            if (s > 0.0) { s = sqrt(s); D[j * LD + j] = s; *s_piv = s; }
            else *s_fail = 1;
        }
        __syncthreads();
        if (*s_fail) return 0;
        if (t > j && t < tw) D[t * LD + j] = s / *s_piv;
        __syncthreads();
    }
    for (int idx = t; idx < T * T; idx += NT) {
        const int x = idx % T, y = idx / T;
        if (x >= y && x < tw) P.S[(size_t)(c0 + y) * P.n + c0 + x] = D[x * LD + y];
    }
    return 1;
}

__global__ __launch_bounds__(NT) void k_llt_diag0(Llt P)
{
    __shared__ double D[T * LD];
    __shared__ double s_piv;
    __shared__ int s_fail;
    const int tw = tile_rows(P, 0);
    load_diag_lower(P, 0, tw, D);
    __syncthreads();
    const int ok = factor_diag(P, 0, tw, D, nullptr, false, &s_fail, &s_piv);
    if (threadIdx.x == 0) flag_write(P.ok, ok);                 // written on either path: the word is stale
}

// Panel K (not the last): row tile R = K + 1 + blockIdx.x against the final diagonal tile.  Thread i owns row r0 + i: its T
// entries one after the other, each dot continued over the tile's columns in ascending k.
__global__ __launch_bounds__(NT) void k_llt_rows(Llt P, int K)
{
    __shared__ double Dp[T * (T + 1) / 2];      // L of the diagonal tile, packed rows: read at uniform addresses only
    __shared__ double O[T * LD];                // row i: the running dots, then L as the columns become final
    if (!flag_read(P.ok)) return;
    const int n = P.n, R = K + 1 + blockIdx.x, c0 = K * T, r0 = R * T, rows = tile_rows(P, R), t = threadIdx.x;
    for (int idx = t; idx < T * T; idx += NT) {
        const int x = idx % T, y = idx / T;
        if (x >= y) Dp[x * (x + 1) / 2 + y] = P.S[(size_t)(c0 + y) * n + c0 + x];
        const int j = idx % T, i = idx / T;
        if (K > 0 && i < rows) O[i * LD + j] = P.S[(size_t)(r0 + i) * n + c0 + j];
    }
    __syncthreads();
    if (t >= rows) return;
    double *o = O + t * LD;
    double a_next = P.S[(size_t)c0 * n + r0 + t];
    for (int j = 0; j < T; ++j) {
        const double a = a_next;
        if (j + 1 < T) a_next = P.S[(size_t)(c0 + j + 1) * n + r0 + t];
        const double *dj = Dp + j * (j + 1) / 2;
        double s = a;
        if (K > 0) {
            double dot = o[j];
            LLT_UNROLL_K
            for (int k = 0; k < j; ++k) dot = dot + o[k] * dj[k];
            s = a - dot;
        } else if (j > 0) {
            double dot = o[0] * dj[0];
            LLT_UNROLL_K
            for (int k = 1; k < j; ++k) dot = dot + o[k] * dj[k];
            s = a - dot;
        }
        const double l = s / dj[j];
        o[j] = l;
        P.S[(size_t)(c0 + j) * n + r0 + t] = l;
    }
}

// Panel K (not the last): trailing tile (R, C), K < C <= R, adds the panel's T products to its running dots, 4 x 4 entries per
// thread with k innermost.  Entry (i, j), i > j, keeps its dot at S[i * n + j]; the diagonal's is x[i].  The workgroup of tile
// (K + 1, K + 1) keeps its dots in LDS instead and factorises the tile.
__global__ __launch_bounds__(NT) void k_llt_update(Llt P, int K)
{
    __shared__ double sm[T * LD + T];
    __shared__ double s_piv;
    __shared__ int s_fail;
    const int R = K + 1 + blockIdx.y, C = K + 1 + blockIdx.x;
    if (C > R) return;
    if (!flag_read(P.ok)) return;
    const int n = P.n, p0 = K * T, r0 = R * T, c0 = C * T, t = threadIdx.x;
    const int lj = 4 * (t % (T / 4)), li = 4 * (t / (T / 4));      // lanes run along j: a dot row is contiguous in S
    const bool next_diag = R == K + 1 && C == K + 1;
    double *As = sm, *Bs = sm + KH * T;
    double acc[4][4];
    if (K > 0)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int gi = r0 + li + a, gj = c0 + lj + b;
                acc[a][b] = 0.0;
                if (gi < n && gi > gj) acc[a][b] = P.S[(size_t)gi * n + gj];
                else if (gi < n && gi == gj) acc[a][b] = P.x[gi];
            }
    for (int h = 0; h < T / KH; ++h) {
        __syncthreads();
        for (int idx = t; idx < KH * T; idx += NT) {
            const int i = idx % T, k = idx / T;
            const size_t col = (size_t)(p0 + h * KH + k) * n;
            As[k * T + i] = r0 + i < n ? P.S[col + r0 + i] : 0.0;
            Bs[k * T + i] = c0 + i < n ? P.S[col + c0 + i] : 0.0;
        }
        __syncthreads();
        int k = 0;
        if (K == 0 && h == 0) {                                 // the dot STARTS as the product for k = 0
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) acc[a][b] = As[li + a] * Bs[lj + b];
            k = 1;
        }
        for (; k < KH; ++k) {
            double av[4], bv[4];
            for (int a = 0; a < 4; ++a) { av[a] = As[k * T + li + a]; bv[a] = Bs[k * T + lj + a]; }
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + av[a] * bv[b];
        }
    }
    if (!next_diag) {
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int gi = r0 + li + a, gj = c0 + lj + b;
                if (gi < n && gi > gj) P.S[(size_t)gi * n + gj] = acc[a][b];
                else if (gi < n && gi == gj) P.x[gi] = acc[a][b];
            }
        return;
    }
    __syncthreads();                                            // the strips are done with: the tile takes their place
    double *D = sm, *dd = sm + T * LD;
    const int tw = tile_rows(P, R);
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const int i = li + a, j = lj + b;
            if (i > j) D[j * LD + i] = acc[a][b];
            else if (i == j) dd[i] = acc[a][b];
        }
    load_diag_lower(P, r0, tw, D);
    __syncthreads();
    if (!factor_diag(P, r0, tw, D, dd, true, &s_fail, &s_piv) && t == 0) flag_write(P.ok, 0);
}

// L y = b.  K = -1: tile 0 alone (y = b through its diagonal tile).  K >= 0: row tile R = K + 1 + blockIdx.x subtracts L[i][j] y_j
// for the panel's final y_j in ascending j; tile K + 1 is complete with that and divides through its own diagonal tile.
__global__ __launch_bounds__(NT) void k_llt_fwd(Llt P, int K)
{
    __shared__ double Ls[T * LD];
    __shared__ double yk[T];
    __shared__ double sh[2];
    const int n = P.n, R = K + 1 + blockIdx.x, r0 = R * T, rows = tile_rows(P, R), t = threadIdx.x;
    if (!flag_read(P.ok)) {
        if (t < rows) P.x[r0 + t] = 0.0;
        return;
    }
    double y = 0.0;
    if (t < rows) y = K <= 0 ? P.b[r0 + t] : P.x[r0 + t];
    if (K >= 0) {
        const int k0 = K * T;
        for (int idx = t; idx < T * T; idx += NT) {
            const int i = idx % T, j = idx / T;
            if (i < rows) Ls[j * LD + i] = P.S[(size_t)(k0 + j) * n + r0 + i];
        }
        if (t < T) yk[t] = P.x[k0 + t];
        __syncthreads();
        if (t < rows)
            for (int j = 0; j < T; ++j) y -= Ls[j * LD + t] * yk[j];
        if (R != K + 1) {
            if (t < rows) P.x[r0 + t] = y;
            return;
        }
        __syncthreads();
    }
    load_diag_lower(P, r0, rows, Ls);
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
        if (t == j) { y = y / Ls[j * LD + j]; sh[j & 1] = y; }
        __syncthreads();
        if (t > j && t < rows) y -= Ls[t * LD + j] * sh[j & 1];
    }
    if (t < rows) P.x[r0 + t] = y;
}

// L^T x = y.  K = nt: the last tile alone.  K < nt: row tile R = blockIdx.x < K subtracts L[j][i] x_j for the panel's final x_j in
// descending j; tile K - 1 is complete with that.
__global__ __launch_bounds__(NT) void k_llt_bwd(Llt P, int K)
{
    __shared__ double Ls[T * LD];
    __shared__ double xk[T];
    __shared__ double sh[2];
    const int n = P.n, R = K == P.nt ? P.nt - 1 : (int)blockIdx.x, r0 = R * T, rows = tile_rows(P, R), t = threadIdx.x;
    if (!flag_read(P.ok)) {
        if (t < rows) P.x[r0 + t] = 0.0;
        return;
    }
    double y = t < rows ? P.x[r0 + t] : 0.0;
    if (K < P.nt) {
        const int k0 = K * T, kw = tile_rows(P, K);
        for (int idx = t; idx < T * T; idx += NT) {
            const int j = idx % T, i = idx / T;                 // entry (k0 + j, r0 + i) of L: lanes run along its column
            if (j < kw) Ls[j * LD + i] = P.S[(size_t)(r0 + i) * n + k0 + j];
        }
        if (t < kw) xk[t] = P.x[k0 + t];
        __syncthreads();
        if (t < rows)
            for (int j = kw - 1; j >= 0; --j) y -= Ls[j * LD + t] * xk[j];
        if (R != K - 1) {
            if (t < rows) P.x[r0 + t] = y;
            return;
        }
        __syncthreads();
    }
    load_diag_lower(P, r0, rows, Ls);
    __syncthreads();
    for (int j = rows - 1; j >= 0; --j) {
        if (t == j) { y = y / Ls[j * LD + j]; sh[j & 1] = y; }
        __syncthreads();
        if (t < j) y -= Ls[j * LD + t] * sh[j & 1];
    }
    if (t < rows) P.x[r0 + t] = y;
}

std::atomic<int> g_last_llt_launches{0};

} // namespace

int orbm_llt_tile(void) { return T; }

int orbm_debug_last_llt_launches(void) { return g_last_llt_launches.load(); }

int orbm_llt_solve_dev(int n, double *S_dev, const double *b_dev, double *x_dev, int32_t *ok_dev, void *stream)
{
    if (n < 1 || n > LLT_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "n outside 1 .. 3,072");
    if (!S_dev || !b_dev || !x_dev || !ok_dev) ORBX_FAIL(ORBX_ERR_ARG, "null pointer");
    ORBX_NEED_DEVICE();
    hipStream_t st = static_cast<hipStream_t>(stream);
    Llt P;
    P.n = n; P.nt = (n + T - 1) / T; P.S = S_dev; P.b = b_dev; P.x = x_dev; P.ok = ok_dev;
    const int nt = P.nt;
    int launches = 0;
    hipLaunchKernelGGL(k_llt_diag0, dim3(1), dim3(NT), 0, st, P); ++launches;
    for (int K = 0; K + 1 < nt; ++K) {
        const unsigned m = (unsigned)(nt - K - 1);
        hipLaunchKernelGGL(k_llt_rows, dim3(m), dim3(NT), 0, st, P, K); ++launches;
        hipLaunchKernelGGL(k_llt_update, dim3(m, m), dim3(NT), 0, st, P, K); ++launches;
    }
    hipLaunchKernelGGL(k_llt_fwd, dim3(1), dim3(NT), 0, st, P, -1); ++launches;
    for (int K = 0; K + 1 < nt; ++K) { hipLaunchKernelGGL(k_llt_fwd, dim3((unsigned)(nt - K - 1)), dim3(NT), 0, st, P, K); ++launches; }
    hipLaunchKernelGGL(k_llt_bwd, dim3(1), dim3(NT), 0, st, P, nt); ++launches;
    for (int K = nt - 1; K >= 1; --K) { hipLaunchKernelGGL(k_llt_bwd, dim3((unsigned)K), dim3(NT), 0, st, P, K); ++launches; }
    ORBX_HIP(hipGetLastError());
    g_last_llt_launches = launches;
    return ORBX_OK;
}
