// orbx_extract_internal.h -- what the extractor's translation units share: orbx_extract.hip (handle, plan driver, reserve,
// batch and one-frame calls) and one unit per stage -- orbx_pyramid.hip, orbx_fast.hip, orbx_octree.hip, orbx_blur.hip,
// orbx_describe.hip -- each a kernel with the host code that plans for it and launches it.
//
// Host interface of a stage unit:
//   int  plan_<stage>(ex, ...)       pure host arithmetic (orbx_plan runs it without a device): fills the fields of `ex`
//                                    the stage's kernel reads; plan_frame (orbx_extract.hip) calls them in order
//   int  prepare_<stage>(ex)         only where a device call at reserve time must name the kernel
//   void launch_<stage>(ex, ..., batch, st)   geometry, variant choice and the profiler bracket of the stage
#ifndef ORBX_EXTRACT_INTERNAL_H
#define ORBX_EXTRACT_INTERNAL_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "common.h"
#include "orbx_internal.h"

namespace orbx_detail {

constexpr int DESC_KPB = 16;   // keypoints per k_describe workgroup: it reads whole chunks of that many selected-keypoint slots

__host__ __device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

#ifdef ORBX_PHASE_TIMING
// development aid (never in the product build): shader-clock time per kernel phase, one record per workgroup (plain
// stores: atomics on shared counters serialise in one L2 channel and the measurement measures itself).
// Per workgroup: 8 phase times (shader clock), [13] = end and [15] = start in the 100 MHz wall clock, [14] = HW_ID.
// Without relocatable device code a __device__ array cannot be shared between units, and each of the four kinds (0 FAST,
// 1 describe, 2 pyramid, 3 octree) belongs to one unit: ORBX_PHASE_UNIT(stage), ahead of the unit's kernels, defines the unit's
// quarter and phases_<stage>(), which copies it out and / or clears it (orbx_debug_phases puts the four together).
int phase_quarter(void *rec, unsigned long long *out, int reset);   // orbx_extract.hip
#define ORBX_PHASE_UNIT(stage) \
    namespace { __device__ unsigned long long g_phase_rec[65536 * 16]; } \
    namespace orbx_detail { int phases_##stage(unsigned long long *out, int reset) { \
        void *p = nullptr; \
        return hipGetSymbolAddress(&p, HIP_SYMBOL(g_phase_rec)) == hipSuccess ? phase_quarter(p, out, reset) : -1; } }
#define ORBX_PH_INIT(K) unsigned long long *const ph_rec = g_phase_rec + ((blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) & 65535u) * 16; \
    if (threadIdx.x == 0) { ph_rec[15] = wall_clock64(); ph_rec[14] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); } \
    __builtin_amdgcn_s_waitcnt(0); unsigned long long ph_t = clock64()   /* the wall clock's own latency stays outside the first phase */
#define ORBX_PH(i, cond) do { if (cond) { const unsigned long long ph_n = clock64(); ph_rec[(i) & 7] = ph_n - ph_t; ph_t = ph_n; } } while (0)
#define ORBX_PH_END(cond) do { if (cond) ph_rec[13] = wall_clock64(); } while (0)   // s_memrealtime is slow: once, at the very end
#define ORBX_PHA(i, cond) do { if (cond) { const unsigned long long ph_n = clock64(); ph_rec[(i) & 7] += ph_n - ph_t; ph_t = ph_n; } } while (0)   // accumulating (loops)
int phases_fast(unsigned long long *out, int reset);
int phases_describe(unsigned long long *out, int reset);
int phases_pyramid(unsigned long long *out, int reset);
int phases_octree(unsigned long long *out, int reset);
#else
#define ORBX_PHASE_UNIT(stage)
#define ORBX_PH_INIT(K) do {} while (0)
#define ORBX_PH(i, cond) do {} while (0)
#define ORBX_PH_END(cond) do {} while (0)
#define ORBX_PHA(i, cond) do {} while (0)
#endif

// XCD-aware (frame, item) mapping for grids of (nitems, nframes) workgroups (speed only,
// never correctness): workgroups are dealt round-robin over the 8 XCDs in dispatch
// order (x fastest), each XCD has its own L2; handing every XCD whole frames lets the
// halos / patches of one frame hit in one L2 instead of being fetched by all eight.
__device__ __forceinline__ void xcd_frame_item(int &frame, int &item)
{
    const int nb = gridDim.x, B = gridDim.y, id = blockIdx.x + nb * blockIdx.y;
    if ((B & 7) == 0) {
        const int x = id & 7, s = id >> 3;
        frame = (s / nb) * 8 + x;
        item = s % nb;
    } else {
        frame = blockIdx.y;
        item = blockIdx.x;
    }
}

// a[23:0] * b[23:0], low 32 bits, as ONE full-rate instruction: the compiler folds __mul24 of values whose range it cannot see back into
// v_mul_lo_u32 (quarter rate)
__device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b)
{
    uint32_t d;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// Dword load at any byte address: gfx950 under amdhsa runs in unaligned-access mode (the compiler itself turns an
// align-1 4-byte copy into one global_load_dword).
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// ... and a 16-byte piece at any byte address (one global_load_dwordx4)
__device__ __forceinline__ uint4 load_u128_unaligned(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// k_fast_cells' tile row of a cell cw px wide: the dwords the LDS tile takes (5 spare bytes, the cell, rounded up) and the
// 16-byte pieces that bring them over -- the last piece reaches up to 12 bytes past the last dword (plan_fast checks where to)
__host__ __device__ __forceinline__ int fast_row_dwords(int cw) { return (cw + 5 + 3) >> 2; }
__host__ __device__ __forceinline__ int fast_row_pieces(int cw) { return (fast_row_dwords(cw) + 3) >> 2; }

inline int cv_round_f(float v) { return (int)lrintf(v); }

// ---- orbx_pyramid.hip: kinds 0 (k_pyr_level0 / _lin) and 1 (k_pyr_chain, or k_pyr_resize per level)
int plan_pyramid(orbx_extractor *ex, int l, std::vector<int2> &xt, std::vector<int4> &yt);   // level l's resize tables and window checks
int plan_chain(orbx_extractor *ex, const std::vector<int2> &xt, const std::vector<int4> &yt); // k_pyr_chain's tiling; needs every level's tables
int prepare_chain(orbx_extractor *ex);
void launch_level0(orbx_extractor *ex, const uint8_t *d_img, int stride, size_t frame_stride, int batch, hipStream_t st);
void launch_pyramid(orbx_extractor *ex, int batch, hipStream_t st);
// ---- orbx_fast.hip: kind 2
int plan_fast(orbx_extractor *ex, int maxcw, int maxch);   // widest / tallest cell of the grid plan_frame laid out
void launch_fast(orbx_extractor *ex, int batch, hipStream_t st);
int debug_fast_pieces(const orbx_extractor *ex, int32_t *out, int cap, int *n);   // orbx_debug_fast_pieces: what the tile load reads, cell by cell
// ---- orbx_octree.hip: kind 3
int plan_octree(orbx_extractor *ex);
int prepare_octree(orbx_extractor *ex);
void launch_octree(orbx_extractor *ex, int batch, hipStream_t st);
// ---- orbx_blur.hip: kind 4
int plan_blur(orbx_extractor *ex, int l);   // level l's tile strips
int prepare_blur(orbx_extractor *ex);
void launch_blur(orbx_extractor *ex, int batch, hipStream_t st);
// ---- orbx_describe.hip: kind 5
int level_slots(const LevelInfo &lv);   // slots of a level in the selected-keypoint array
void launch_describe(orbx_extractor *ex, int batch, hipStream_t st);

} // namespace orbx_detail

#endif // ORBX_EXTRACT_INTERNAL_H
