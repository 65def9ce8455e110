// orbm_llt.hip -- dense Cholesky solve of a system wider than one workgroup can factorise (include/orbslam_hip.h,
// orbm_llt_solve_dev), and the same solve over the live tiles of a tile envelope (orbm_llt_env_solve_dev).
// S = L L^T in place on the lower triangle, L y = b, L^T x = y, in T x T tiles over many workgroups, and every number by the
// operations of k_ba_solve (orbm_ba.hip) in k_ba_solve's order:
//   L[i][j] = (a[i][j] - dot) / L[j][j],  dot = L[i][0] L[j][0], then dot = dot + L[i][k] L[j][k] for k = 1 .. j - 1 ascending
// The order is per ENTRY, so a tiled, right-looking factorisation keeps it: every lower entry (i, j) that is not final yet owns ONE
// running dot; when panel K's columns are final every trailing entry adds the panel's T products in ascending k.  Row tile R holds
// the tiles (R, first[R]) .. (R, R); the running dot of tile (R, C) is ASSIGNED by its first live panel max(first[R], first[C]), and a
// tile no panel reaches has no dot.  The dense solver is the envelope solver with first[R] = 0.
//   k_llt_diag0    the first diagonal tile, one workgroup
//   k_llt_rows     panel K: a workgroup per row tile of the panel solves its rows against the FINAL diagonal tile
//   k_llt_update   panel K: a workgroup per trailing tile adds the panel's products to its running dots; the workgroup of the NEXT
//                  diagonal tile then holds that tile's complete dots and factorises it on the spot
//   k_llt_fwd / k_llt_bwd   the substitutions, a launch per panel: every row tile subtracts the panel's T final unknowns in order;
//                  the tile that is complete with that divides through its own diagonal tile
// ONE body per kernel, a template over where a tile and its running dot live (Dense, Env below); the arithmetic is written once.
// A diagonal tile is written by ONE workgroup, in a launch in which no other workgroup reads it (the launch BEFORE the one whose
// workgroups solve against it): no workgroup waits for another, ordering is the stream's, every loop is bounded by n, T or a count of
// the plan.  4 nt - 1 launches for nt = ceil(n / T) tiles, fewer where a panel of the envelope has no row tile.  A pivot that is not
// > 0 clears *ok; every later launch reads it first and does nothing, the substitutions write x = 0 instead.  Plain double multiplies
// and adds (-ffp-contract=off), no MFMA, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../../include/orbslam_hip.h"
#include "common.h"
#include "orbm_llt_env.h"

namespace {

constexpr int T = 64;                   // tile edge
constexpr int NT = 256;                 // threads per workgroup; thread t < T owns row (or column) t of the tile in the serial parts
constexpr int LD = T + 1;               // row stride of a tile in LDS: rows read by lanes fall on distinct banks
constexpr int KH = 32;                  // the update's strips go through LDS in two halves of the panel
constexpr int LLT_MAXN = 3072;
constexpr int ENV_MAXN = 28672;
constexpr int ENV_MAXTILES = 8192;
// the k loops of the serial parts: the two LDS reads of a step do not depend on the running sum, so eight steps' reads are issued
// together and only the adds stay a chain (the order of the adds is the source's: nothing is reassociated)
#define LLT_UNROLL_K _Pragma("unroll 8")
static_assert(T % KH == 0 && NT == (T / 4) * (T / 4), "4 x 4 entries per thread");

// Where a tile and its running dot live, and which row tiles a panel has.  tile(R, C): entry (0, 0) of tile (R, C), column-major,
// ld() doubles from a column to the next.  dots(R, C)(i, j): the running dot of the tile's entry (i, j) (the tile's part of the
// address is taken once per workgroup, not once per entry).  rows_in(K), row(K, idx): panel K's row tiles (R > K with
// first(R) <= K), ascending.  ALONE: the update's grid may carry one more row (below).

// The n x n column-major square: the dot of entry (gi, gj), gi > gj, at the mirrored place S[gi * n + gj] of the strict upper
// triangle, the diagonal's in x, which is free until the substitutions.  Every tile is live.
struct Dense {
    static constexpr bool ALONE = false;
    int n, nt;
    double *S;
    const double *b;
    double *x;
    int *ok;
    __device__ size_t ld() const { return (size_t)n; }
    __device__ double *tile(int R, int C) const { return S + (size_t)C * T * n + (size_t)R * T; }
    struct Dots {
        double *s, *xd;                 // the dot of the tile's entry (0, 0); x at the tile's first row on the diagonal, or null
        size_t n;
        __device__ double *operator()(int i, int j) const { return xd && i == j ? xd + i : s + (size_t)i * n + j; }
    };
    __device__ Dots dots(int R, int C) const { return Dots{S + (size_t)R * T * n + (size_t)C * T, R == C ? x + R * T : nullptr, (size_t)n}; }
    __device__ int first(int) const { return 0; }
    __device__ int rows_in(int K) const { return nt - K - 1; }
    __device__ int row(int K, int idx) const { return K + 1 + idx; }
};

// Packed tiles of T x T doubles in A at the plan's tile numbers; the dots in W at the tile's own number, ROW-major (the update's
// lanes run along j), the diagonal's on the diagonal.
struct Env {
    static constexpr bool ALONE = true;
    int n, nt;
    double *A, *W;
    const double *b;
    double *x;
    int *ok;
    LltEnvView v;
    __device__ size_t ld() const { return T; }
    __device__ double *tile(int R, int C) const { return A + (size_t)v.tile_index(R, C) * (T * T); }
    struct Dots {
        double *w;
        __device__ double *operator()(int i, int j) const { return w + (i * T + j); }
    };
    __device__ Dots dots(int R, int C) const { return Dots{W + (size_t)v.tile_index(R, C) * (T * T)}; }
    __device__ int first(int R) const { return v.first[R]; }
    __device__ int rows_in(int K) const { return v.row_start[K + 1] - v.row_start[K]; }
    __device__ int row(int K, int idx) const { return v.rows[v.row_start[K] + idx]; }
};

// the flag: one workgroup may clear it while others of the same launch read it (either value makes them do what they should: the
// launch's results are not used once it is 0), so both sides are relaxed atomics and not plain accesses
__device__ __forceinline__ int flag_read(int *ok) { return __hip_atomic_load(ok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void flag_write(int *ok, int v) { __hip_atomic_store(ok, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class P> __device__ __forceinline__ int tile_rows(const P &p, int R) { const int r = p.n - R * T; return r < T ? r : T; }
// the panel that assigns the dots of tile (R, C)
template <class P> __device__ __forceinline__ int first_panel(const P &p, int R, int C) { const int a = p.first(R), b = p.first(C); return a > b ? a : b; }

// D[x][y] (x >= y) = entry (x, y) of the diagonal tile at `tile` (column-major, ld doubles from a column to the next), all threads;
// the upper part of D is left alone
__device__ __forceinline__ void load_diag_lower(const double *tile, size_t ld, int tw, double *D)
{
    for (int idx = threadIdx.x; idx < T * T; idx += NT) {
        const int x = idx % T, y = idx / T;
        if (x >= y && x < tw) D[x * LD + y] = tile[y * ld + x];
    }
}

// The diagonal tile, tw wide, in D: the lower part holds a, and with has_dots D[j][r] (r > j) the running dot of entry (r, j)
// and dd[r] the diagonal's.  Thread t owns row t.  Leaves L in the lower part of D and writes it to the tile (as load_diag_lower
// reads it); 0 (in every thread) at a pivot that is not > 0, with nothing written.
__device__ int factor_diag(double *tile, size_t ld, int tw, double *D, const double *dd, bool has_dots, int *s_fail, double *s_piv)
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
        if (x >= y && x < tw) tile[y * ld + x] = D[x * LD + y];
    }
    return 1;
}

// Diagonal tile Kd from a alone: tile 0 (which writes the flag on either path: the word is stale), or a tile whose row starts at
// itself (first(Kd) = Kd), which only ever clears it.
template <class P> __device__ void diag_alone(const P &p, int Kd, double *D, int *s_fail, double *s_piv)
{
    double *tile = p.tile(Kd, Kd);
    const int tw = tile_rows(p, Kd);
    load_diag_lower(tile, p.ld(), tw, D);
    __syncthreads();
    const int ok = factor_diag(tile, p.ld(), tw, D, nullptr, false, s_fail, s_piv);
    if (threadIdx.x == 0 && (Kd == 0 || !ok)) flag_write(p.ok, ok);
}

template <class P> __global__ __launch_bounds__(NT) void k_llt_diag0(P p)
{
    __shared__ double D[T * LD];
    __shared__ double s_piv;
    __shared__ int s_fail;
    diag_alone(p, 0, D, &s_fail, &s_piv);
}

// Panel K (not the last): row tile R = the blockIdx.x-th of the panel's against the final diagonal tile.  Thread i owns row i of the
// tile: its T entries one after the other, each dot continued over the tile's columns in ascending k.
template <class P> __global__ __launch_bounds__(NT) void k_llt_rows(P p, int K)
{
    __shared__ double Dp[T * (T + 1) / 2];      // L of the diagonal tile, packed rows: read at uniform addresses only
    __shared__ double O[T * LD];                // row i: the running dots, then L as the columns become final
    if (!flag_read(p.ok)) return;
    const int R = p.row(K, blockIdx.x), rows = tile_rows(p, R), t = threadIdx.x;
    const bool dots = K > first_panel(p, R, K);
    const size_t ld = p.ld();
    const double *Dt = p.tile(K, K);
    double *At = p.tile(R, K);
    const auto dot = p.dots(R, K);
    for (int idx = t; idx < T * T; idx += NT) {
        const int x = idx % T, y = idx / T;
        if (x >= y) Dp[x * (x + 1) / 2 + y] = Dt[y * ld + x];
        const int j = idx % T, i = idx / T;
        if (dots && i < rows) O[i * LD + j] = *dot(i, j);
    }
    __syncthreads();
    if (t >= rows) return;
    double *o = O + t * LD;
    double a_next = At[t];
    for (int j = 0; j < T; ++j) {
        const double a = a_next;
        if (j + 1 < T) a_next = At[(j + 1) * ld + t];
        const double *dj = Dp + j * (j + 1) / 2;
        double s = a;
        if (dots) {
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
        At[j * ld + t] = l;
    }
}

// Panel K (not the last): the trailing tiles are the pairs (R, C), C <= R, of the panel's m row tiles: grid (max(m, 1), m + alone),
// the upper half exits.  A tile adds the panel's T products to its running dots, 4 x 4 entries per thread with k innermost.  The next
// diagonal tile (K + 1, K + 1) is the list's first pair when the panel reaches it: its workgroup keeps the dots in LDS instead and
// factorises the tile.  When the panel does not reach it (first(K + 1) = K + 1, ALONE policies only) the grid has one more row, whose
// first workgroup factorises that tile from a alone.
template <class P> __global__ __launch_bounds__(NT) void k_llt_update(P p, int K)
{
    __shared__ double sm[T * LD + T];
    __shared__ double s_piv;
    __shared__ int s_fail;
    const int m = p.rows_in(K);
    if (P::ALONE && (int)blockIdx.y == m) {
        if (blockIdx.x == 0 && flag_read(p.ok)) diag_alone(p, K + 1, sm, &s_fail, &s_piv);
        return;
    }
    if ((int)blockIdx.x >= m) return;
    const int R = p.row(K, blockIdx.y), C = p.row(K, blockIdx.x);
    if (C > R) return;
    if (!flag_read(p.ok)) return;
    const int r0 = R * T, c0 = C * T, rr = tile_rows(p, R), rc = tile_rows(p, C), t = threadIdx.x;
    const int lj = 4 * (t % (T / 4)), li = 4 * (t / (T / 4));      // lanes run along j: a dot row is contiguous
    const bool next_diag = R == K + 1 && C == K + 1, assign = K == first_panel(p, R, C);
    const size_t ld = p.ld();
    const double *Ar = p.tile(R, K), *Ac = p.tile(C, K);
    const auto dot = p.dots(R, C);
    double *As = sm, *Bs = sm + KH * T;
    double acc[4][4];
    if (!assign)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int i = li + a, j = lj + b;
                acc[a][b] = i < rr && r0 + i >= c0 + j ? *dot(i, j) : 0.0;
            }
    for (int h = 0; h < T / KH; ++h) {
        __syncthreads();
        for (int idx = t; idx < KH * T; idx += NT) {
            const int i = idx % T, k = idx / T;
            const size_t col = (size_t)(h * KH + k) * ld;
            As[k * T + i] = i < rr ? Ar[col + i] : 0.0;
            Bs[k * T + i] = i < rc ? Ac[col + i] : 0.0;
        }
        __syncthreads();
        int k = 0;
        if (assign && h == 0) {                                 // the dot STARTS as the product for the panel's first column
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
                const int i = li + a, j = lj + b;
                if (i < rr && r0 + i >= c0 + j) *dot(i, j) = acc[a][b];
            }
        return;
    }
    __syncthreads();                                            // the strips are done with: the tile takes their place
    double *D = sm, *dd = sm + T * LD;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const int i = li + a, j = lj + b;
            if (i > j) D[j * LD + i] = acc[a][b];
            else if (i == j) dd[i] = acc[a][b];
        }
    double *tile = p.tile(R, R);
    load_diag_lower(tile, ld, rr, D);
    __syncthreads();
    if (!factor_diag(tile, ld, rr, D, dd, true, &s_fail, &s_piv) && t == 0) flag_write(p.ok, 0);
}

// L y = b.  K = -1: tile 0 alone (y = b through its diagonal tile).  K >= 0: the panel's row tiles subtract L[i][j] y_j for its final
// y_j in ascending j; one more workgroup stands for tile K + 1 when the list does not hold it.  Tile K + 1 is complete either way and
// divides through its own diagonal tile.  A row tile starts from b at its first panel.
template <class P> __global__ __launch_bounds__(NT) void k_llt_fwd(P p, int K)
{
    __shared__ double Ls[T * LD];
    __shared__ double yk[T];
    __shared__ double sh[2];
    const bool panel = K >= 0 && (int)blockIdx.x < p.rows_in(K);
    const int R = panel ? p.row(K, blockIdx.x) : K + 1;
    const int r0 = R * T, rows = tile_rows(p, R), t = threadIdx.x;
    const size_t ld = p.ld();
    if (!flag_read(p.ok)) {
        if (t < rows) p.x[r0 + t] = 0.0;
        return;
    }
    double y = 0.0;
    if (t < rows) y = !panel || K == p.first(R) ? p.b[r0 + t] : p.x[r0 + t];
    if (panel) {
        const int k0 = K * T;
        const double *Lt = p.tile(R, K);
        for (int idx = t; idx < T * T; idx += NT) {
            const int i = idx % T, j = idx / T;
            if (i < rows) Ls[j * LD + i] = Lt[j * ld + i];
        }
        if (t < T) yk[t] = p.x[k0 + t];
        __syncthreads();
        if (t < rows)
            for (int j = 0; j < T; ++j) y -= Ls[j * LD + t] * yk[j];
        if (R != K + 1) {
            if (t < rows) p.x[r0 + t] = y;
            return;
        }
        __syncthreads();
    }
    load_diag_lower(p.tile(R, R), ld, rows, Ls);
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
        if (t == j) { y = y / Ls[j * LD + j]; sh[j & 1] = y; }
        __syncthreads();
        if (t > j && t < rows) y -= Ls[t * LD + j] * sh[j & 1];
    }
    if (t < rows) p.x[r0 + t] = y;
}

// L^T x = y.  K = nt: the last tile alone.  K < nt: tile R = first(K) + blockIdx.x < K subtracts L[j][i] x_j for the panel's final x_j
// in descending j through the live tile (K, R); when row K has no such tile (first(K) = K) the one workgroup stands for tile K - 1,
// which is complete either way.
template <class P> __global__ __launch_bounds__(NT) void k_llt_bwd(P p, int K)
{
    __shared__ double Ls[T * LD];
    __shared__ double xk[T];
    __shared__ double sh[2];
    const bool panel = K < p.nt && p.first(K) < K;
    const int R = K == p.nt ? p.nt - 1 : panel ? p.first(K) + (int)blockIdx.x : K - 1;
    const int r0 = R * T, rows = tile_rows(p, R), t = threadIdx.x;
    const size_t ld = p.ld();
    if (!flag_read(p.ok)) {
        if (t < rows) p.x[r0 + t] = 0.0;
        return;
    }
    double y = t < rows ? p.x[r0 + t] : 0.0;
    if (panel) {
        const int k0 = K * T, kw = tile_rows(p, K);
        const double *Lt = p.tile(K, R);
        for (int idx = t; idx < T * T; idx += NT) {
            const int j = idx % T, i = idx / T;                 // entry (k0 + j, r0 + i) of L: lanes run along its column
            if (j < kw) Ls[j * LD + i] = Lt[i * ld + j];
        }
        if (t < kw) xk[t] = p.x[k0 + t];
        __syncthreads();
        if (t < rows)
            for (int j = kw - 1; j >= 0; --j) y -= Ls[j * LD + t] * xk[j];
        if (R != K - 1) {
            if (t < rows) p.x[r0 + t] = y;
            return;
        }
        __syncthreads();
    }
    load_diag_lower(p.tile(R, R), ld, rows, Ls);
    __syncthreads();
    for (int j = rows - 1; j >= 0; --j) {
        if (t == j) { y = y / Ls[j * LD + j]; sh[j & 1] = y; }
        __syncthreads();
        if (t < j) y -= Ls[j * LD + t] * sh[j & 1];
    }
    if (t < rows) p.x[r0 + t] = y;
}

// The launch chain of either solver.  rows_of(K): the row tiles of panel K; first(R) as in the policy.  Returns the launches.
template <class P, class RowsOf, class First> int llt_launch(const P &p, hipStream_t st, RowsOf rows_of, First first)
{
    const int nt = p.nt;
    const dim3 wg(NT);
    int launches = 0;
    hipLaunchKernelGGL(k_llt_diag0<P>, dim3(1), wg, 0, st, p); ++launches;
    for (int K = 0; K + 1 < nt; ++K) {
        const unsigned m = (unsigned)rows_of(K), alone = first(K + 1) == K + 1;
        if (m) { hipLaunchKernelGGL(k_llt_rows<P>, dim3(m), wg, 0, st, p, K); ++launches; }   // skipped when empty, never an empty grid
        hipLaunchKernelGGL(k_llt_update<P>, dim3(m ? m : 1, m + alone), wg, 0, st, p, K); ++launches;
    }
    hipLaunchKernelGGL(k_llt_fwd<P>, dim3(1), wg, 0, st, p, -1); ++launches;
    for (int K = 0; K + 1 < nt; ++K) {
        const unsigned m = (unsigned)rows_of(K) + (first(K + 1) == K + 1);
        hipLaunchKernelGGL(k_llt_fwd<P>, dim3(m), wg, 0, st, p, K); ++launches;
    }
    hipLaunchKernelGGL(k_llt_bwd<P>, dim3(1), wg, 0, st, p, nt); ++launches;
    for (int K = nt - 1; K >= 1; --K) {
        const unsigned m = (unsigned)(K - first(K));
        hipLaunchKernelGGL(k_llt_bwd<P>, dim3(m ? m : 1), wg, 0, st, p, K); ++launches;
    }
    return launches;
}

// n and first[] as both entries check them; *live = the live tiles
int env_check(int n, const int32_t *first, int *live)
{
    if (n < 1 || n > ENV_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "n outside 1 .. 28,672");
    if (!first) ORBX_FAIL(ORBX_ERR_ARG, "null pointer");
    const int nt = (n + T - 1) / T;
    long long tiles = 0;
    for (int R = 0; R < nt; ++R) {
        if (first[R] < 0 || first[R] > R) ORBX_FAIL(ORBX_ERR_ARG, "first[R] outside 0 .. R");
        tiles += R - first[R] + 1;
    }
    if (tiles > ENV_MAXTILES) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 live tiles");
    *live = (int)tiles;
    return ORBX_OK;
}

// rows_of[K] = row tiles R > K with first[R] <= K (nt entries, the last one 0)
void env_row_counts(int nt, const int32_t *first, int *rows_of)
{
    for (int K = 0; K < nt; ++K) rows_of[K] = 0;
    for (int R = 1; R < nt; ++R)
        for (int K = first[R]; K < R; ++K) ++rows_of[K];        // one step per live off-diagonal tile
}

std::atomic<int> g_last_llt_launches{0};

} // namespace

int orbm_llt_solve_dev(int n, double *S_dev, const double *b_dev, double *x_dev, int32_t *ok_dev, void *stream)
{
    if (n < 1 || n > LLT_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "n outside 1 .. 3,072");
    if (!S_dev || !b_dev || !x_dev || !ok_dev) ORBX_FAIL(ORBX_ERR_ARG, "null pointer");
    ORBX_NEED_DEVICE();
    const int nt = (n + T - 1) / T;
    const Dense p{n, nt, S_dev, b_dev, x_dev, ok_dev};
    const int launches = llt_launch(p, static_cast<hipStream_t>(stream), [&](int K) { return nt - K - 1; }, [](int) { return 0; });
    ORBX_HIP(hipGetLastError());
    g_last_llt_launches = launches;
    return ORBX_OK;
}

int orbm_llt_env_plan(int n, const int32_t *first, int32_t *off, int32_t *row_start, int32_t *rows, int32_t *trail_start, int32_t *trail,
                      int32_t *counts)
{
    int live = 0;
    if (const int e = env_check(n, first, &live)) return e;
    const int nt = (n + T - 1) / T;
    int nrows = 0, ntrail = 0, launches = 1 + 2 * nt;           // the first diagonal tile, and a launch per tile in either substitution
    if (off) off[0] = 0;
    for (int R = 0; R < nt; ++R)
        if (off) off[R + 1] = off[R] + R - first[R] + 1;
    for (int K = 0; K < nt; ++K) {
        if (row_start) row_start[K] = nrows;
        if (trail_start) trail_start[K] = ntrail;
        const int r_begin = nrows;
        for (int R = K + 1; R < nt; ++R)
            if (first[R] <= K) {
                if (rows) rows[nrows] = R;
                ++nrows;
                int c = 0;
                for (int C = K + 1; C <= R; ++C)
                    if (first[C] <= K) {
                        if (trail) { trail[2 * (ntrail + c)] = R; trail[2 * (ntrail + c) + 1] = C; }
                        ++c;
                    }
                ntrail += c;
            }
        if (K + 1 < nt) launches += nrows > r_begin ? 2 : 1;    // the row tiles if there are any; the trailing tiles and the next diagonal tile
    }
    if (row_start) row_start[nt] = nrows;
    if (trail_start) trail_start[nt] = ntrail;
    if (counts) { counts[0] = live; counts[1] = nrows; counts[2] = ntrail; counts[3] = launches; }
    return ORBX_OK;
}

int orbm_llt_env_solve_dev(int n, const int32_t *first, const int32_t *plan_dev, double *A_dev, double *W_dev, const double *b_dev,
                           double *x_dev, int32_t *ok_dev, void *stream)
{
    int live = 0;
    if (const int e = env_check(n, first, &live)) return e;
    if (!plan_dev || !A_dev || !W_dev || !b_dev || !x_dev || !ok_dev) ORBX_FAIL(ORBX_ERR_ARG, "null pointer");
    ORBX_NEED_DEVICE();
    const int nt = (n + T - 1) / T;
    int rows_of[(ENV_MAXN + T - 1) / T];
    env_row_counts(nt, first, rows_of);
    const Env p{n, nt, A_dev, W_dev, b_dev, x_dev, ok_dev, LltEnvView(plan_dev, nt)};
    const int launches = llt_launch(p, static_cast<hipStream_t>(stream), [&](int K) { return rows_of[K]; }, [&](int R) { return first[R]; });
    ORBX_HIP(hipGetLastError());
    g_last_llt_launches = launches;
    return ORBX_OK;
}

int orbm_llt_tile(void) { return T; }

int orbm_debug_last_llt_launches(void) { return g_last_llt_launches.load(); }
