// fem_internal.h -- what fem.hip shares with the bundle solver that runs the Levenberg hook inside its own kernel (orbm_pose_nr.hip):
// the device functions that fix the BITS of f = K a and of the strain energy -- the 16-lanes-per-row sum, the wave / block sum of
// the energy -- and an accessor for the device arrays a model keeps resident for the hook.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fem_hip.h"

namespace fem_detail {

// f = K*a in float, ascending column order per row (= the dense row sum of MultiplyMatricesEigen with exact zeros skipped, and the
// oracle's left-to-right sum, bit for bit).  16 lanes per row: they fetch 16 entries of the row side by side -- value, column,
// a[column] -- and lane 0 of the group adds the 16 products IN ORDER, the products handed down the group one lane per step
// (DPP row_shl:1).  The order of the additions is the reference's; only the memory round trips run side by side.  (One thread
// walking its row alone waited for memory at every entry: 34 us for 3,756 rows of ~117 entries, most of an LM trial.)
// Entries past the row's end contribute +0.0f, which leaves a float sum that started at +0.0f unchanged (it can never be -0.0f).
__device__ __forceinline__ void fem_chunk_add16(float &s, float p)
{
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        s += p;                                                                                   // lane 0: + product j of the chunk
        p = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0x101, 0xf, 0xf, true));   // row_shl:1
    }
}
__device__ __forceinline__ float fem_row_sum16(const float *__restrict__ v, const int *__restrict__ lcol, const float *__restrict__ am,
                                               int k0, int k1, int sub)
{
    float s = 0.0f;
    for (int kb = k0; kb < k1; kb += 16) {
        const int k = kb + sub;
        float p = 0.0f;
        if (k < k1) p = v[k] * am[lcol[k]];
        fem_chunk_add16(s, p);
    }
    return s;   // valid in lane 0 of the 16-lane group
}
// R rows per 16-lane group side by side (entries [k0[j], k1[j]) of row j; an empty range for no row), each row's sum exactly
// fem_row_sum16's: its chunks in order, a chunk's products in order.  A row that has ended goes on adding +0.0f while a longer one
// finishes, which changes nothing (above).  For a lone workgroup that walks a whole matrix (k_pose_nr): the R rows' memory round
// trips and their R chains of additions overlap, where one row at a time waits for each in turn.
template <int R>
__device__ __forceinline__ void fem_row_sum16_rows(const float *__restrict__ v, const int *__restrict__ lcol, const float *__restrict__ am,
                                                   const int (&k0)[R], const int (&k1)[R], int sub, float (&s)[R])
{
    int kb[R];
    bool more = false;
#pragma unroll
    for (int j = 0; j < R; ++j) { kb[j] = k0[j]; s[j] = 0.0f; more |= kb[j] < k1[j]; }
    while (more) {
        float p[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int k = kb[j] + sub;
            p[j] = 0.0f;
            if (k < k1[j]) p[j] = v[k] * am[lcol[k]];
        }
        more = false;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            fem_chunk_add16(s[j], p[j]);
            kb[j] += 16;
            more |= kb[j] < k1[j];
        }
    }
}

// Sum over the wave, the same value in every lane, in a fixed order: four DPP row_shr steps leave each row of 16 lanes' total in its
// last lane, the four row totals are read into scalars and added row 0 .. 3.  No LDS round trips: the xor butterfly through
// ds_bpermute (12 of them per f64 sum, each step waiting for the last) was 2 us of the 5 the coarse correction added per iteration.
template <int N> __device__ __forceinline__ double dpp_shr_f64(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x110 + N, 0xf, 0xf, true);         // row_shr:N, 0 from beyond the row
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x110 + N, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v += dpp_shr_f64<1>(v);
    v += dpp_shr_f64<2>(v);
    v += dpp_shr_f64<4>(v);
    v += dpp_shr_f64<8>(v);
    return ((readlane_f64(v, 15) + readlane_f64(v, 31)) + readlane_f64(v, 47)) + readlane_f64(v, 63);
}
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    v = wave_sum_f64(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    return t;
}

// sE = |a^T f| and nsE = sE / int(Ksize / 3) from the block total of the 256-thread strided double sum (k_fem_energy, k_fem_matvec_energy)
__device__ __forceinline__ void strain_energy_of(double s, int ndof, float &sE, float &nsE)
{
    float e = (float)s;
    if (e < 0.0f) e = -e;
    sE = e;
    nsE = e / (float)(ndof / 3);
}

// The hook's front half for ONE mesh by one workgroup of nthreads threads (k_fem_trial_a_fused, k_pose_nr): the vertex estimates ->
// float top layer (GetPointCoordinates' cast), the derived mid-edge / barycentre nodes (FEA2.cc:1746-1775; by one thread in the
// reference's order when one builds on another), a = uf - u0, the Dirichlet entries of ImposeDirichletEncastre_a.  top: 3 nTop
// floats, a: ndof = 6 nTop floats, in device memory or LDS.  The steps wait for each other at workgroup barriers, so every thread of
// the workgroup must call it; the caller adds the barrier behind the last step if it reads a.
__device__ __forceinline__ void trial_displacement(const double *__restrict__ p, int npoints, const int *__restrict__ derived, int nder,
                                                   int sequential, float *t, const float *__restrict__ u0, float *am,
                                                   const int *__restrict__ ids, int nids, float klarge, int tid, int nthreads)
{
    const int nTop = npoints + nder, ndof = 6 * nTop;
    for (int i = tid; i < 3 * npoints; i += nthreads) t[i] = (float)p[i];
    __syncthreads();
    if (nder) {
        if (sequential) {
            if (tid == 0)
                for (int d = 0; d < nder; ++d) {
                    const int *e = derived + 4 * d;
                    for (int k = 0; k < 3; ++k)
                        t[3 * (npoints + d) + k] = e[0] == 2 ? (t[3 * e[1] + k] + t[3 * e[2] + k]) / 2
                                                             : (t[3 * e[1] + k] + t[3 * e[2] + k] + t[3 * e[3] + k]) / 3;
                }
        } else {
            for (int i = tid; i < 3 * nder; i += nthreads) {
                const int d = i / 3, k = i - 3 * d;
                const int *e = derived + 4 * d;
                t[3 * (npoints + d) + k] = e[0] == 2 ? (t[3 * e[1] + k] + t[3 * e[2] + k]) / 2
                                                     : (t[3 * e[1] + k] + t[3 * e[2] + k] + t[3 * e[3] + k]) / 3;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < ndof; i += nthreads) {
        const float u = u0[i];
        am[i] = (i < 3 * nTop ? t[i] : u) - u;
    }
    __syncthreads();
    for (int q = tid; q < nids * 3; q += nthreads) am[3 * (ids[q / 3] - 1) + q % 3] = 1 / klarge;
}

// The device arrays of a single-mesh model whose hook is set up (fem_trial_setup): K as CSR, u0, the derived-node table
// {2 | 3, i0, i1, i2} (sequential: one derived node builds on another, keep the reference's order) and the Dirichlet ids.
struct TrialView {
    const float *vals, *u0;
    const int *lcol, *rowptr, *derived, *ids;
    int ndof, npoints, nder, nids, sequential;
    float klarge;
    hipStream_t stream;
};
// false: no model, a batch of meshes, or fem_trial_setup has not run
__attribute__((visibility("hidden"))) bool trial_view(const fem_model *m, TrialView *v);

} // namespace fem_detail
