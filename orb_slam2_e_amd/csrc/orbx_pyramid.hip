// orbx_pyramid.hip -- the extractor's image pyramid (ComputePyramid, ORBextractor.cc:1115-1140): level 0 with its border
// (k_pyr_level0 / k_pyr_level0_lin), and the levels above it either one launch per level (k_pyr_resize; k_pyr_resize_small where its
// copy rule does not hold) or, for small batches, all in one launch (k_pyr_chain).  What the kernels require of the host stands
// below them: the resize tables, the window checks and the copy rule (plan_pyramid), the cut of a row into waves (resize_split),
// the chain's tiling (plan_chain), and the launch geometry (launch_level0, launch_pyramid).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "orbx_extract_internal.h"

using namespace orbx_detail;

ORBX_PHASE_UNIT(pyramid)

namespace {

// ------------------------------------------------------------------ pyramid
// Both pyramid kernels are latency-bound (two dependent global loads per output),
// so every thread produces 4 pixels (one dword store) in PYR_ROWS rows and keeps
// all of their loads in flight at once.  The 19-px REFLECT_101 border of a resized
// level is a copy of pixels the same wave has just computed (k_pyr_resize), stored
// in the same pass; level 0 and the tiny levels read it through the reflected coordinate.
// Rows per thread, round 4 (same-box A/B of the pipelined step, three rounds each): 4 -> 0.2495 ms, 6 -> 0.2474, 8 -> 0.2447-0.2471,
// 10 -> 0.2536, 16 -> 0.2568.  A resize launch alone is no faster with 8 (8.7 against 8.1 us: half the waves, each twice as long) -- but
// the chain then holds half the wave slots while it waits for memory, and the other contexts' kernels get them.
constexpr int PYR_ROWS = 8;

// Level 0: copyMakeBorder(image, temp, 19,19,19,19, BORDER_REFLECT_101), ORBextractor.cc:1135.
__global__ __launch_bounds__(64) void k_pyr_level0(const uint8_t *__restrict__ img, int img_stride,
                                                   size_t img_frame_stride, uint8_t *__restrict__ pyr,
                                                   size_t frame_bytes, LevelInfo lv, int aligned)
{
    const int xw = blockIdx.x * 64 + threadIdx.x;
    if (xw * 4 >= lv.stride) return;
    const int f = blockIdx.z, px0 = xw * 4 - PADX;
    const bool inner = aligned && px0 >= 0 && px0 + 4 <= lv.w;
    int sx[4];
    uint32_t keep = 0; // bytes inside [-EDGE, w+EDGE); the others (row padding) read a clamped column and are masked to 0
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int px = px0 + b;
        sx[b] = reflect101(min(max(px, -EDGE), lv.w + EDGE - 1), lv.w);
        keep |= (px >= -EDGE && px < lv.w + EDGE) ? 0xffu << (8 * b) : 0u;
    }
    uint32_t out[PYR_ROWS];
#pragma unroll
    for (int r = 0; r < PYR_ROWS; ++r) {
        const int row = blockIdx.y * PYR_ROWS + r;
        out[r] = 0;
        if (row < lv.h + 2 * EDGE) {
            const uint8_t *src = img + (size_t)f * img_frame_stride + (size_t)reflect101(row - EDGE, lv.h) * img_stride;
            if (inner) {
                out[r] = *reinterpret_cast<const uint32_t *>(src + px0);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) out[r] |= (uint32_t)src[sx[b]] << (8 * b);
                out[r] &= keep;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PYR_ROWS; ++r) {
        const int row = blockIdx.y * PYR_ROWS + r;
        if (row < lv.h + 2 * EDGE)
            *reinterpret_cast<uint32_t *>(pyr + (size_t)f * frame_bytes + lv.off + (size_t)row * lv.stride + xw * 4) = out[r];
    }
}

// The same for images whose width is a multiple of 8 (and whose rows are dword-aligned), without a divergent wave: the
// padded level is (h + 38) rows x pp = w / 8 interior pieces of 8 bytes -- every one a straight copy from a (reflected)
// source row, numbered row-major and dealt out 64 x 4 per wave (8 bytes per lane and load: the texture addresser's sweet
// spot) -- plus nb border dwords per row (the 19 px either side), which are put together byte by byte through the reflected
// column by waves of their own.  The dword form above had the border lanes in the first and last wave of every row group:
// both paths executed by two waves of three.  inv_pp / inv_nb = ceil(2^32 / pp), ceil(2^32 / nb): exact quotients.
__global__ __launch_bounds__(64) void k_pyr_level0_lin(const uint8_t *__restrict__ img, int img_stride, size_t img_frame_stride,
                                                       uint8_t *__restrict__ pyr, size_t frame_bytes, LevelInfo lv, int pp,
                                                       unsigned inv_pp, int nblk_int, int nb, unsigned inv_nb, int nleft)
{
    int f, bx;
    xcd_frame_item(f, bx);          // grid (workgroups per frame, frames): a frame's pyramid is made by one XCD, launch after launch
    const int lane = threadIdx.x, rows = lv.h + 2 * EDGE;
    const uint8_t *src = img + (size_t)f * img_frame_stride;
    uint8_t *dst = pyr + (size_t)f * frame_bytes + lv.off;
    if (bx < nblk_int) {
        uint2 v[4];
        int row[4], pc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = min(bx * 256 + u * 64 + lane, rows * pp - 1);   // past the end: the last piece again
            row[u] = (int)(((unsigned long long)(unsigned)p * inv_pp) >> 32);
            pc[u] = p - row[u] * pp;
            __builtin_memcpy(&v[u], src + (uint32_t)(reflect101(row[u] - EDGE, lv.h) * img_stride + 8 * pc[u]), 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            *reinterpret_cast<uint2 *>(dst + (uint32_t)(row[u] * lv.stride + PADX + 8 * pc[u])) = v[u];
    } else {
        const int q = (bx - nblk_int) * 64 + lane;
        if (q >= rows * nb) return;
        const int row = (int)(((unsigned long long)(unsigned)q * inv_nb) >> 32), k = q - row * nb;
        const int xw = k < nleft ? ((PADX - EDGE) >> 2) + k : ((PADX + lv.w) >> 2) + (k - nleft);   // dword of the padded row
        const uint8_t *s = src + (uint32_t)(reflect101(row - EDGE, lv.h) * img_stride);
        uint32_t out = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int px = xw * 4 - PADX + b;
            const uint32_t val = s[reflect101(min(max(px, -EDGE), lv.w + EDGE - 1), lv.w)];
            out |= (px >= -EDGE && px < lv.w + EDGE) ? val << (8 * b) : 0u;   // row padding stays 0
        }
        *reinterpret_cast<uint32_t *>(dst + (uint32_t)(row * lv.stride + xw * 4)) = out;
    }
}

// Level l from level l-1: cv::resize INTER_LINEAR 8U fixed point
// + REFLECT_101 border.  xt[dx] = {sx, a0 | a1<<16}, yt[dy] = {sy0, sy1, b0, b1}:
// OpenCV's coefficient tables, built on the host.
//
// Interior dword groups (4 pixels with 0 <= x < w, no reflection): the source columns of such a group are
// non-decreasing and span at most 8 bytes (the host checks it per level), so each source row is ONE unaligned
// 8-byte load and a pixel's pair (S[sx], S[sx+1]) is one v_perm_b32 into two u16 halves, times (a0, a1) one
// v_dot2_u32_u16.  The last group of a row whose width is no multiple of 4 reads clamped table entries for the pixels past
// w - 1 (same window, bytes replaced by border bytes before the store).  k_pyr_resize_small takes every pixel one by one
// through the reflected coordinate instead.
// (b (r >> 4)) >> 16 = floor((b 2^12) (r & ~15) / 2^32): both factors are below 2^24 (b <= 2048, r <= 255 * 2048), so
// it is one v_mul_hi_u32_u24 after the mask instead of shift, multiply, shift.  bs = b << 12.
// (written as asm: from the masked 64-bit product the compiler makes v_mul_hi_u32, a quarter-rate instruction -- 64 of them were
// a fifth of the kernel's VALU time)
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b)   // (a[23:0] * b[23:0]) >> 32
{
    uint32_t d;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ uint32_t resize_vertical(int r0, int r1, uint32_t bs0, uint32_t bs1)
{
    const uint32_t t0 = mulhi_u24(bs0, (uint32_t)r0 & 0xfffff0u);
    const uint32_t t1 = mulhi_u24(bs1, (uint32_t)r1 & 0xfffff0u);
    const uint32_t v = (t0 + t1 + 2) >> 2;
    return v > 255u ? 255u : v;
}
typedef unsigned short pyr_u16x2 __attribute__((ext_vector_type(2)));
// Thread -> work.  A level with the copy rule (plan_pyramid: w, h >= 20 and the 8-byte window holds) is resampled ONCE: image rows
// 0 .. h-1 only, in row groups of PYR_ROWS, and of a padded row the dwords xlo .. xhi, lane = dword.  A row is cut from the left
// into full waves of 64 dwords (resize_split); what is left over (fewer than 64) is a TILE of the row's LAST 16, 32 or 64 dwords x
// 4, 2 or 1 row groups per wave, which stores the leftover dwords and every dword of the right border (a full wave then stores
// interior dwords only; the other dwords of the tile are computed for the border's sake).  So the first wave of a row holds the
// left border and pixels 0 .. 20, the last one -- tile or full wave -- the right border and the 20-odd pixels it mirrors.
// Line ownership: the cuts are at dwords xlo + 64 k = 3 + 64 k, so the 64-byte line that holds a cut is stored by the two waves
// that meet there (full wave k-1 and full wave k, or the last full wave and the tile), every other line by one wave.  A cut at
// whole lines (four lines per wave) was measured: the same WRITE_SIZE (54.8 MB per 64-frame step either way, 1.06 x the padded
// bytes -- the L2 merges the halves), but 25,344 waves and 15.2 M vector instructions per step instead of 24,384 and 13.1 M,
// because a row of 16 k + a few dwords then costs a whole extra wave per row group; profiles/pyramid_border_copy_notes.md.
//   interior dword (4 pixels, 0 <= x < w)   the 8-byte-window arithmetic above, stored as computed
//   border dword, and the dword that straddles the right image edge (w % 4 != 0)   REFLECT_101 says byte x = -k is pixel k and
//       x = w-1+k is pixel w-1-k: its (up to) four source pixels lie in two neighbouring groups {q, q+1} of the same wave, so the
//       lane fetches those two finished dwords (ds_bpermute) and picks its bytes with one v_perm_b32 -- selector and source lanes
//       are set up once per wave; bytes of row padding select the constant 0.  Only the first and the last wave of a row do this
//       (a wave-uniform branch); their interior lanes fetch themselves with the identity selector.  A border lane computes the
//       group it is clamped to beside its neighbours (same cache lines) and its own result is dropped.
//   border ROWS   the lane that holds image row y also stores it to padded row EDGE - y (1 <= y <= 19) and to padded row
//       EDGE + 2 (h-1) - y (h-20 <= y <= h-2): the same registers, another row address; no row-table entry is read for a border row.
// The column table carries up to three clamped entries past w (plan_pyramid) so that the last, partial group reads its int4 pair
// like every other.  Dwords of pure row padding (outside the 19-px border) are not written: the workspace is zeroed once.
struct ResizeLane {
    const uint8_t *src;      // level l-1, pixel (sx0, 0) of the lane's window
    uint8_t *out;            // level l, the lane's dword of padded row 0
    uint32_t coef[4], sel[4];
    uint32_t bsel;           // byte selector of the exchange (edge waves)
    int lane_lo, lane_hi;    // its two source lanes, as ds_bpermute addresses
    bool store;
};
// NR rows from image row y0 on.  UNIFORM: y0 is the same in all lanes (full waves): row table through the scalar cache, the row
// conditions scalar branches; otherwise (tiles) a vector load and predicated stores -- the row table then lies in vector registers,
// and a tile takes its row group in two halves to stay within the 64 registers that let 8 waves share a SIMD
template <bool UNIFORM, int NR>
__device__ __forceinline__ void resize_rows(const ResizeLane &L, int y0, bool edge, int src_stride, int dst_stride, int h,
                                            const int4 *__restrict__ yt)
{
    if (UNIFORM) y0 = __builtin_amdgcn_readfirstlane(y0);
    int4 yy[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) yy[r] = yt[min(y0 + r, h - 1)];
    uint2 w0[NR], w1[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        __builtin_memcpy(&w0[r], L.src + (uint32_t)((yy[r].x + EDGE) * src_stride), 8);
        __builtin_memcpy(&w1[r], L.src + (uint32_t)((yy[r].y + EDGE) * src_stride), 8);
    }
    uint32_t out[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        out[r] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int r0 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(pyr_u16x2, __builtin_amdgcn_perm(w0[r].y, w0[r].x, L.sel[b])),
                                                       __builtin_bit_cast(pyr_u16x2, L.coef[b]), 0u, false);
            const int r1 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(pyr_u16x2, __builtin_amdgcn_perm(w1[r].y, w1[r].x, L.sel[b])),
                                                       __builtin_bit_cast(pyr_u16x2, L.coef[b]), 0u, false);
            out[r] |= resize_vertical(r0, r1, (uint32_t)yy[r].z << 12, (uint32_t)yy[r].w << 12) << (8 * b);
        }
    }
    if (edge) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(L.lane_lo, (int)out[r]);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(L.lane_hi, (int)out[r]);
            out[r] = __builtin_amdgcn_perm(hi, lo, L.bsel);
        }
    }
    if (L.store) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int y = y0 + r;
            if (y < h) {
                *reinterpret_cast<uint32_t *>(L.out + (uint32_t)((y + EDGE) * dst_stride)) = out[r];
                if (y >= 1 && y <= EDGE) *reinterpret_cast<uint32_t *>(L.out + (uint32_t)((EDGE - y) * dst_stride)) = out[r];
                if (y >= h - 1 - EDGE && y <= h - 2) *reinterpret_cast<uint32_t *>(L.out + (uint32_t)((EDGE + 2 * (h - 1) - y) * dst_stride)) = out[r];
            }
        }
    }
}
__global__ __launch_bounds__(64) void k_pyr_resize(uint8_t *__restrict__ pyr, size_t frame_bytes, LevelInfo src,
                                                   LevelInfo dst, const int2 *__restrict__ xt,
                                                   const int4 *__restrict__ yt, int nfull, int tws, int dtile, int rpw)
{
    int f, bx;
    xcd_frame_item(f, bx);
    const int tid = threadIdx.x;
    ORBX_PH_INIT(2);
    const int nrg = (dst.h + PYR_ROWS - 1) / PYR_ROWS, nrgw = (nrg + rpw - 1) / rpw;
    const int xlo = (PADX - EDGE) >> 2, xhi = (PADX + dst.w + EDGE - 1) >> 2; // first / last dword that holds border or image bytes
    const bool tile = bx >= nfull * nrgw;      // full waves first (wave kx of the row, row groups rw * rpw ..), then the tiles
#ifdef ORBX_PHASE_TIMING
    if (tid == 0) { ph_rec[12] = dst.w; ph_rec[11] = tile ? 0 : 1; }
#endif
    int d0, sub, rg;                            // the wave's first dword of the padded row; lane's place in its row; row group
    bool edge;
    if (!tile) {
        const int rw = bx / nfull, kx = bx - rw * nfull;
        d0 = xlo + 64 * kx; sub = tid; rg = rw * rpw;
        edge = kx == 0 || (tws == 0 && kx == nfull - 1);
    } else {
        const int tw = 1 << tws;
        sub = tid & (tw - 1);
        d0 = xhi + 1 - tw; rg = ((bx - nfull * nrgw) << (6 - tws)) + (tid >> tws);
        edge = true;
    }
    const int D = d0 + sub;
    ResizeLane L;
    L.store = tile ? D >= dtile : D < dtile;   // dtile: the first dword the tiles store (xhi + 1: no tiles)
    // every lane computes a group (the border lanes the nearest one: in-bounds loads, result unused) and stays active for the exchange
    const int g = min(max(D - PADX / 4, 0), ((dst.w + 3) >> 2) - 1);
    const int4 xa = *reinterpret_cast<const int4 *>(xt + 4 * g), xb = *reinterpret_cast<const int4 *>(xt + 4 * g + 2);
    const int sx0 = xa.x;
    L.coef[0] = (uint32_t)xa.y; L.coef[1] = (uint32_t)xa.w; L.coef[2] = (uint32_t)xb.y; L.coef[3] = (uint32_t)xb.w;
    // selector {byte o, 0, byte o+1, 0} of the 8-byte window, o = sx - sx0
    L.sel[0] = 0x0c010c00u; L.sel[1] = 0x0c010c00u + (uint32_t)(xa.z - sx0) * 0x00010001u;
    L.sel[2] = 0x0c010c00u + (uint32_t)(xb.x - sx0) * 0x00010001u; L.sel[3] = 0x0c010c00u + (uint32_t)(xb.z - sx0) * 0x00010001u;
    L.bsel = 0; L.lane_lo = 0;
    if (edge) {
        // the dword's pixels through the mirror (one fold: w >= 20 > EDGE), the lower of the two groups that hold them, and each
        // byte's place in that pair of dwords
        int s[4], smin = 1 << 30;
        bool in[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int p = 4 * D - PADX + b;
            in[b] = p >= -EDGE && p < dst.w + EDGE;
            s[b] = p < 0 ? -p : (p >= dst.w ? 2 * (dst.w - 1) - p : p);
            smin = in[b] ? min(smin, s[b]) : smin;
        }
        const int qlo = smin == (1 << 30) ? 0 : smin >> 2;
#pragma unroll
        for (int b = 0; b < 4; ++b) L.bsel |= (in[b] ? (uint32_t)(s[b] - 4 * qlo) : 0x0cu) << (8 * b);
        L.lane_lo = (PADX / 4 + qlo - d0 + (tid - sub)) * 4;      // (byte address of ds_bpermute; the host checked that the pair lies in this wave's row)
    }
    L.lane_hi = (L.lane_lo + 4) & 252;
    L.src = pyr + (size_t)f * frame_bytes + src.off + PADX + sx0;
    L.out = pyr + (size_t)f * frame_bytes + dst.off + D * 4;
    // A full wave works on one row group at a time: the row-table entries are wave-uniform and come through the scalar cache; the
    // column table is read once and serves all rpw row groups of the wave.  The kernel's time is a wave's life (three dependent
    // memory round trips, 4-6 us) times the number of wave generations, and a level's wave count is what the host sets through
    // rpw so that one generation holds them all.
    if (tile && tws != 6) {
        resize_rows<false, PYR_ROWS / 2>(L, rg * PYR_ROWS, true, src.stride, dst.stride, dst.h, yt);      // (rows past the last: clamped, nothing stored)
        resize_rows<false, PYR_ROWS / 2>(L, rg * PYR_ROWS + PYR_ROWS / 2, true, src.stride, dst.stride, dst.h, yt);
    } else {
        const int nj = tile ? 1 : rpw;          // (a tile as wide as a wave is one row group: uniform like a full wave)
        for (int j = 0; j < nj; ++j) {
            if ((rg + j) * PYR_ROWS >= dst.h) break;
            resize_rows<true, PYR_ROWS>(L, (rg + j) * PYR_ROWS, edge, src.stride, dst.stride, dst.h, yt);
        }
    }
    ORBX_PH(1, tid == 0);   // column table, source rows, arithmetic, exchange, stores
    ORBX_PH(2, tid == 0);
    ORBX_PH_END(tid == 0);
}

// The levels the copy rule does not cover (narrower or lower than 20 px: the mirror folds more than once; or a scale at which a
// group's source columns do not fit the 8-byte window): every dword of the padded level, border rows and columns included, pixel by
// pixel through the reflected coordinate.  A tile is 2^tw_shift dwords x 64 >> tw_shift row groups of the padded level; ntw > 1 (a row
// wider than a wave) only with tw_shift = 6.  No level of a 640 x 480 or 1242 x 375 pyramid takes it.
__global__ __launch_bounds__(64) void k_pyr_resize_small(uint8_t *__restrict__ pyr, size_t frame_bytes, LevelInfo src,
                                                         LevelInfo dst, const int2 *__restrict__ xt,
                                                         const int4 *__restrict__ yt, int ndw, int tw_shift, int ntw, int tail_window)
{
    int f, bx;
    xcd_frame_item(f, bx);
    const int tid = threadIdx.x;
    ORBX_PH_INIT(2);
#ifdef ORBX_PHASE_TIMING
    if (tid == 0) { ph_rec[12] = dst.w; ph_rec[11] = 0; }
#endif
    const int xlo = (PADX - EDGE) >> 2, xhi = (PADX + dst.w + EDGE - 1) >> 2; // first / last dword that holds border or image bytes
    const int tr = bx / ntw;
    const int col = ((bx - tr * ntw) << tw_shift) + (tid & ((1 << tw_shift) - 1));
    const int rowg = (tr << (6 - tw_shift)) + (tid >> tw_shift);
    if (col >= ndw) return;
    const int xw = xlo + col;
    if (xw > xhi || rowg * PYR_ROWS >= dst.h + 2 * EDGE) return;
    const uint8_t *base = pyr + (size_t)f * frame_bytes + src.off + PADX;
    uint32_t out[PYR_ROWS];
    {
        int4 yy[PYR_ROWS];
#pragma unroll
        for (int r = 0; r < PYR_ROWS; ++r) {
            const int row = rowg * PYR_ROWS + r;
            yy[r] = yt[reflect101((row < dst.h + 2 * EDGE ? row : 0) - EDGE, dst.h)];
        }
        // no per-pixel branches: pixels outside [-EDGE, w+EDGE) (row padding) take the column of a clamped coordinate and
        // are masked out of the stored dword
        const int px0 = xw * 4 - PADX;
        int sxs[4], a0[4], a1[4];
        uint32_t keep = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int px = px0 + b;
            const bool in = px >= -EDGE && px < dst.w + EDGE;
            const int2 xx = xt[reflect101(min(max(px, -EDGE), dst.w + EDGE - 1), dst.w)];
            sxs[b] = xx.x; a0[b] = xx.y & 0xffff; a1[b] = xx.y >> 16;
            keep |= in ? 0xffu << (8 * b) : 0u;
        }
        if (tail_window) {
            // The four source columns of a dword lie within 7 bytes (the host checks it per level, reflected and clamped columns
            // included): one 8-byte window from the smallest of them serves all four -- 8 loads per lane instead of 64 single bytes.
            const int smin = min(min(sxs[0], sxs[1]), min(sxs[2], sxs[3]));
            uint32_t sel[4], coef[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sel[b] = 0x0c010c00u + (uint32_t)(sxs[b] - smin) * 0x00010001u;   // {byte o, 0, byte o+1, 0}
                coef[b] = (uint32_t)a0[b] | ((uint32_t)a1[b] << 16);
            }
            uint2 w0[PYR_ROWS], w1[PYR_ROWS];
#pragma unroll
            for (int r = 0; r < PYR_ROWS; ++r) {
                __builtin_memcpy(&w0[r], base + (uint32_t)((yy[r].x + EDGE) * src.stride + smin), 8);
                __builtin_memcpy(&w1[r], base + (uint32_t)((yy[r].y + EDGE) * src.stride + smin), 8);
            }
#pragma unroll
            for (int r = 0; r < PYR_ROWS; ++r) {
                out[r] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int r0 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(pyr_u16x2, __builtin_amdgcn_perm(w0[r].y, w0[r].x, sel[b])),
                                                               __builtin_bit_cast(pyr_u16x2, coef[b]), 0u, false);
                    const int r1 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(pyr_u16x2, __builtin_amdgcn_perm(w1[r].y, w1[r].x, sel[b])),
                                                               __builtin_bit_cast(pyr_u16x2, coef[b]), 0u, false);
                    out[r] |= resize_vertical(r0, r1, (uint32_t)yy[r].z << 12, (uint32_t)yy[r].w << 12) << (8 * b);
                }
                out[r] &= keep;
            }
        } else
#pragma unroll
        for (int r = 0; r < PYR_ROWS; ++r) {
            const uint8_t *S0 = base + (size_t)(yy[r].x + EDGE) * src.stride;
            const uint8_t *S1 = base + (size_t)(yy[r].y + EDGE) * src.stride;
            out[r] = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int r0 = __mul24(S0[sxs[b]], a0[b]) + __mul24(S0[sxs[b] + 1], a1[b]);
                const int r1 = __mul24(S1[sxs[b]], a0[b]) + __mul24(S1[sxs[b] + 1], a1[b]);
                out[r] |= resize_vertical(r0, r1, (uint32_t)yy[r].z << 12, (uint32_t)yy[r].w << 12) << (8 * b);
            }
            out[r] &= keep;
        }
    }
    ORBX_PH(1, tid == 0 && out[0] != 0x12345678u);   // column table, source rows, arithmetic
#pragma unroll
    for (int r = 0; r < PYR_ROWS; ++r) {
        const int row = rowg * PYR_ROWS + r;
        if (row < dst.h + 2 * EDGE)
            *reinterpret_cast<uint32_t *>(pyr + (size_t)f * frame_bytes + dst.off + (uint32_t)(row * dst.stride + xw * 4)) = out[r];
    }
    ORBX_PH(2, tid == 0);
    ORBX_PH_END(tid == 0);
}

// Levels 1 .. n-1 of the pyramid in ONE launch -- the form SMALL batches take (launch_pyramid: <= 6 frames, the live tracker's one frame
// per call: 22 us against the seven dependent per-level launches' 52; in the pipelined 64-frame step it was slower than they are,
// profiles/r04_notes.md, and is not used there).  A workgroup carries one spatial tile through all levels in LDS: it loads
// its rectangle of level 0, computes from it its rectangle of level 1 (the same fixed-point arithmetic, 4 pixels per lane from an
// 8-byte source window -- taken from three aligned LDS dwords), stores the part of the padded level 1 it owns (border pixels through
// the reflected coordinate, as the per-level kernel does), computes level 2 from level 1, and so on.  The rectangles (host table,
// plan_chain) are what the tile owns at a level plus what its deeper levels read: neighbours overlap by a few pixels per level and
// recompute them (1.3-1.5 x the arithmetic of the exact chain), and nobody waits for anybody.
__device__ __forceinline__ int chain_pitch(int nw) { return ((nw + 15) & ~15) + 16; }
__global__ __launch_bounds__(256) void k_pyr_chain(uint8_t *__restrict__ pyr, size_t frame_bytes, const LevelInfo *__restrict__ L, int nlevels,
                                                   const ChainTile *__restrict__ tiles, const uint4 *__restrict__ tabs,
                                                   const int2 *__restrict__ tab_span, int ldsA, int ldsB)
{
    extern __shared__ __align__(16) uint8_t chain_lds[];
    const int tid = threadIdx.x, f = blockIdx.y;
    ORBX_PH_INIT(2);
#ifdef ORBX_PHASE_TIMING
    if (tid == 0) { ph_rec[12] = 0; ph_rec[11] = 1; ph_rec[1] = ph_rec[2] = ph_rec[3] = 0; }
#endif
    const ChainTile &T = tiles[blockIdx.x];
    uint8_t *const fp = pyr + (size_t)f * frame_bytes;
    // the tile's coefficient tables, prepared by the host as one block (plan_chain): for every level the rows {sy0 | sy1 << 16,
    // b0 | b1 << 16} and then the columns {sx, a0 | a1 << 16} of its rectangle, source coordinates relative to the source rectangle.
    // The rectangles and the levels' geometry are staged too (read per level through the scalar cache they were a dependent memory
    // round trip at the top of every level)
    uint4 *const s_rect = reinterpret_cast<uint4 *>(chain_lds + ldsA + ldsB);          // [MAXL] ChainRect, [MAXL] {w, h, stride, off}
    int2 *const s_tab = reinterpret_cast<int2 *>(s_rect + 2 * MAXL);
    const int2 span = tab_span[blockIdx.x];      // first 16-byte unit, units
    if (tid < MAXL) s_rect[tid] = reinterpret_cast<const uint4 *>(&T)[tid];
    else if (tid < 2 * MAXL) s_rect[tid] = *reinterpret_cast<const uint4 *>(&L[tid - MAXL]);
    auto rect_at = [&](int l) {
        uint4 v = s_rect[l];
        v.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.x); v.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.y);
        v.z = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.z); v.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.w);
        return __builtin_bit_cast(ChainRect, v);
    };
    struct Geo { int w, h, stride, off; };
    auto geo_at = [&](int l) {
        uint4 v = s_rect[MAXL + l];
        Geo g;
        g.w = __builtin_amdgcn_readfirstlane((int)v.x); g.h = __builtin_amdgcn_readfirstlane((int)v.y);
        g.stride = __builtin_amdgcn_readfirstlane((int)v.z); g.off = __builtin_amdgcn_readfirstlane((int)v.w);
        return g;
    };
    {   // level 0: the rectangle in 16-byte pieces (nx0 % 4 == 0: dword-aligned in memory; the columns past nw up to the pitch are read
        // too: they lie inside the padded row), all of a lane's pieces in flight together; the tables travel meanwhile
        const ChainRect r0 = T.r[0];
        const LevelInfo l0 = L[0];
        const int p16 = chain_pitch(r0.nw) >> 4, n = p16 * r0.nh;
        const uint8_t *src = fp + l0.off + PADX + r0.nx0 + (size_t)(r0.ny0 + EDGE) * l0.stride;
        for (int i = tid; i < span.y; i += 256) reinterpret_cast<uint4 *>(s_tab)[i] = tabs[span.x + i];
        for (int i0 = tid; i0 < n; i0 += 4 * 256) {
            uint4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = min(i0 + 256 * k, n - 1), row = i / p16, c = i - row * p16;
                __builtin_memcpy(&v[k], src + (uint32_t)(row * l0.stride + 16 * c), 16);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + 256 * k < n) reinterpret_cast<uint4 *>(chain_lds)[i0 + 256 * k] = v[k];
        }
    }
    __syncthreads();
    int nytot = 0;
    for (int l = 1; l < nlevels; ++l) nytot += rect_at(l).nh;
    const int2 *const s_yt = s_tab, *const s_xt = s_tab + ((nytot + 1) & ~1);
    ORBX_PH(0, tid == 0);    // tables + level 0 in LDS
    int yo = 0, xo = 0;
    ChainRect rp = rect_at(0);
    for (int l = 1; l < nlevels; ++l) {
        const ChainRect rc = rect_at(l);
        const Geo lv = geo_at(l);
        const uint8_t *src = chain_lds + ((l - 1) & 1 ? ldsA : 0);
        uint8_t *dst = chain_lds + (l & 1 ? ldsA : 0);
        const int pp = chain_pitch(rp.nw), pc = chain_pitch(rc.nw);
        uint8_t *const gout = fp + lv.off;
        // ---- compute the rectangle: lane = a group of 4 columns x a band of consecutive rows (G groups side by side, G a power of two,
        // 256 / G bands).  A source row's horizontal pass (4 pixels) stays in registers: consecutive output rows share source rows
        // (sy1 of one is sy0 of the next four times out of five), so a row is read and interpolated 1.2 times instead of 2.  A dword
        // that the tile owns and that holds four interior pixels goes to memory straight from the registers.
        const int ngrp = (rc.nw + 3) >> 2;
        int gs = 0;
        while ((1 << gs) < ngrp) ++gs;
        const int g = tid & ((1 << gs) - 1), band = tid >> gs, nband = 256 >> gs;
        const int rb = (rc.nh + nband - 1) / nband, r_lo = band * rb, r_hi = min(r_lo + rb, (int)rc.nh);
        if (g < ngrp && r_lo < r_hi) {
            const int2 *xg = s_xt + xo + 4 * g;
            const int2 x0 = xg[0], x1 = xg[1], x2 = xg[2], x3 = xg[3];
            const uint32_t coef[4] = {(uint32_t)x0.y, (uint32_t)x1.y, (uint32_t)x2.y, (uint32_t)x3.y};
            const int col0 = x0.x, a4 = col0 >> 2, o = col0 & 3;
            const uint32_t sel[4] = {0x0c010c00u, 0x0c010c00u + (uint32_t)(x1.x - col0) * 0x00010001u,
                                     0x0c010c00u + (uint32_t)(x2.x - col0) * 0x00010001u, 0x0c010c00u + (uint32_t)(x3.x - col0) * 0x00010001u};
            const int2 *yl = s_yt + yo;
            struct H4 { int v[4]; };
            auto horiz = [&](int srow) {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(src + srow * pp) + a4;
                const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
                const uint32_t wx = __builtin_amdgcn_alignbyte(d1, d0, o), wy = __builtin_amdgcn_alignbyte(d2, d1, o);
                H4 h;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    h.v[b] = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(pyr_u16x2, __builtin_amdgcn_perm(wy, wx, sel[b])),
                                                         __builtin_bit_cast(pyr_u16x2, coef[b]), 0u, false);
                return h;
            };
            // the dword of this group in the padded row, and whether the tile stores it from here
            const int gx = rc.nx0 + 4 * g, xw = (PADX + gx) >> 2;
            const bool own_x = xw >= rc.oxw0 && xw < rc.oxw1 && gx + 3 < lv.w;
            int prev = -1;
            H4 hp = {{0, 0, 0, 0}};
            for (int r = r_lo; r < r_hi; ++r) {
                const int2 yy = yl[r];
                const int s0 = yy.x & 0xffff, s1 = (int)((uint32_t)yy.x >> 16);
                const H4 h0 = s0 == prev ? hp : horiz(s0);
                const H4 h1 = s1 == s0 ? h0 : horiz(s1);
                hp = h1; prev = s1;
                const uint32_t bs0 = ((uint32_t)yy.y & 0xffffu) << 12, bs1 = ((uint32_t)yy.y >> 16) << 12;
                uint32_t out = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) out |= resize_vertical(h0.v[b], h1.v[b], bs0, bs1) << (8 * b);
                *reinterpret_cast<uint32_t *>(dst + r * pc + 4 * g) = out;
                const int row = rc.ny0 + r + EDGE;
                if (own_x && row >= rc.or0 && row < rc.or1) *reinterpret_cast<uint32_t *>(gout + (uint32_t)(row * lv.stride + 4 * xw)) = out;
            }
        }
        __syncthreads();
        ORBX_PHA(1, tid == 0);   // compute (all levels)
        // ---- what is left of the tile's share of the padded level: the border (reflected coordinates) -- rows above / below the image
        // in full, beside the image the dwords that are not four interior pixels.  Lane = a dword of the padded row
        const int ndw = rc.oxw1 - rc.oxw0, nrow = rc.or1 - rc.or0;
        const int ilo = PADX >> 2, ihi = (PADX + lv.w) >> 2;           // dwords [ilo, ihi) hold four interior pixels each
        const bool side = rc.oxw0 < ilo || rc.oxw1 > ihi, cap = rc.or0 < EDGE || rc.or1 > lv.h + EDGE;
        if (ndw > 0 && nrow > 0 && (side || cap)) {
            int ws = 0;
            while ((1 << ws) < ndw) ++ws;
            const int c = tid & ((1 << ws) - 1), r1st = tid >> ws, wpass = 256 >> ws;
            if (c < ndw) {
                const int xw = rc.oxw0 + c, px0 = xw * 4 - PADX;
                const bool interior = xw >= ilo && xw < ihi;
                int cx[4]; uint32_t keep = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    int px = min(max(px0 + b, -EDGE), lv.w + EDGE - 1);
                    px = px < 0 ? -px : (px >= lv.w ? 2 * (lv.w - 1) - px : px);       // one fold is enough: |px| <= EDGE < w
                    cx[b] = px - rc.nx0;
                    keep |= (px0 + b >= -EDGE && px0 + b < lv.w + EDGE) ? 0xffu << (8 * b) : 0u;
                }
                for (int r = r1st; r < nrow; r += wpass) {
                    const int row = rc.or0 + r, yy0 = row - EDGE;
                    const bool inrow = yy0 >= 0 && yy0 < lv.h;
                    if (interior && inrow) continue;                                   // stored from the registers above
                    const int y = yy0 < 0 ? -yy0 : (yy0 >= lv.h ? 2 * (lv.h - 1) - yy0 : yy0);
                    const uint8_t *sr = dst + (y - rc.ny0) * pc;
                    uint32_t v;
                    if (interior) v = *reinterpret_cast<const uint32_t *>(sr + cx[0]);   // nx0 % 4 == 0: an aligned dword
                    else v = ((uint32_t)sr[cx[0]] | ((uint32_t)sr[cx[1]] << 8) | ((uint32_t)sr[cx[2]] << 16) | ((uint32_t)sr[cx[3]] << 24)) & keep;
                    *reinterpret_cast<uint32_t *>(gout + (uint32_t)(row * lv.stride + 4 * xw)) = v;
                }
            }
        }
        // (no barrier here: the next level reads `dst`, which nobody writes any more, and writes the other buffer, which nobody
        // reads any more -- its last readers passed the barrier above)
        yo += rc.nh; xo += (rc.nw + 3) & ~3;
        rp = rc;
        ORBX_PHA(2, tid == 0);   // border stores (all levels; thread 0's share)
    }
    ORBX_PH_END(tid == 0);
}

// OpenCV resize coefficient tables for one axis.
void resize_axis(int dn, int sn, std::vector<int> &ofs, std::vector<int> &c0, std::vector<int> &c1)
{
    const double inv_scale = (double)dn / sn, scale = 1. / inv_scale;
    ofs.resize(dn); c0.resize(dn); c1.resize(dn);
    for (int d = 0; d < dn; ++d) {
        float fv = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(fv);
        fv -= s;
        ofs[d] = s;
        const int a0 = cv_round_f((1.f - fv) * 2048.f), a1 = cv_round_f(fv * 2048.f);
        c0[d] = a0 > 32767 ? 32767 : a0;
        c1[d] = a1 > 32767 ? 32767 : a1;
    }
}

// k_pyr_resize's cut of a padded row of width w: nfull waves of 64 dwords from dword xlo on, and for what is left (fewer than 64)
// a tile of the row's last 2^tws dwords (16, 32 or 64: 4, 2 or 1 row groups per wave), which stores from dword dtile on: the
// leftover, and the straddling and right border dwords where the last full wave reaches into them.  tws = 0: nothing is left, and the
// last full wave holds the right border (dtile = xhi + 1).
void resize_split(int w, int &nfull, int &tws, int &dtile)
{
    const int xlo = (PADX - EDGE) >> 2, xhi = (PADX + w + EDGE - 1) >> 2, ndw = xhi - xlo + 1;
    nfull = ndw / 64;
    const int rem = ndw - 64 * nfull;
    tws = rem == 0 ? 0 : rem <= 16 ? 4 : rem <= 32 ? 5 : 6;
    dtile = rem == 0 ? xhi + 1 : std::min(xlo + 64 * nfull, PADX / 4 + (w >> 2));
}

// Whether every border dword (and the straddling one) of such a row finds the two groups its bytes come from in its own wave's
// row -- the kernel's own lane arithmetic, dword by dword -- and every other wave holds interior dwords only.  True for every
// w >= 20 (the left border needs groups 0 .. 5, ten dwords behind xlo; the right border the last seven groups, and the last wave's
// row is the row's last 16 dwords at least); checked all the same, so that another PADX or EDGE one day cannot make a lane fetch
// from a lane that holds something else.
bool resize_pairs_in_wave(int w)
{
    int nfull, tws, dtile;
    resize_split(w, nfull, tws, dtile);
    const int xlo = (PADX - EDGE) >> 2, xhi = (PADX + w + EDGE - 1) >> 2, ngc = (w + 3) >> 2;
    if (tws && (dtile < xhi + 1 - (1 << tws) || dtile < xlo)) return false;
    for (int D = xlo; D <= xhi; ++D) {
        const bool tile = D >= dtile;
        const int kx = (D - xlo) / 64;
        if (!tile && kx != 0 && !(tws == 0 && kx == nfull - 1)) {      // a wave between the edges stores what it computed: interior dwords only
            if (D < PADX / 4 || 4 * (D - PADX / 4) + 3 >= w) return false;
            continue;
        }
        const int d0 = tile ? xhi + 1 - (1 << tws) : xlo + 64 * kx, d1 = tile ? xhi + 1 : d0 + 64;
        int smin = 1 << 30, smax = -1;
        for (int b = 0; b < 4; ++b) {
            const int p = 4 * D - PADX + b;
            if (p < -EDGE || p >= w + EDGE) continue;
            const int s = p < 0 ? -p : (p >= w ? 2 * (w - 1) - p : p);
            if (s < 0 || s >= w) return false;
            smin = std::min(smin, s); smax = std::max(smax, s);
        }
        if (smax < 0) return false;
        const int qlo = smin >> 2, qhi = smax >> 2;
        if (qhi > qlo + 1 || qhi >= ngc) return false;
        if (PADX / 4 + qlo < d0 || PADX / 4 + qhi >= d1) return false;
    }
    return true;
}

} // namespace

namespace orbx_detail {

// Level l's resize tables from level l-1 (appended to xt / yt, which become d_xt / d_yt), and which kernel serves the level:
// resize_nxi (the interior groups' 8-byte source windows hold), resize_copy (k_pyr_resize's copy rule holds; no level of a
// 640 x 480 or 1242 x 375 pyramid fails it, and the planner accepts no level under 62 px a side) and, for k_pyr_resize_small,
// resize_tailwin (every dword of the padded row, border included, keeps its source columns in an 8-byte window).
int plan_pyramid(orbx_extractor *ex, int l, std::vector<int2> &xt, std::vector<int4> &yt)
{
    LevelInfo &lv = ex->lv[l];
    if (xt.size() & 1) xt.push_back(make_int2(0, 0));   // every level's table 16-byte aligned (int4 reads in k_pyr_resize)
    lv.xtab = (int)xt.size(); lv.ytab = (int)yt.size();
    if (l == 0) return ORBX_OK;
    const LevelInfo &sv = ex->lv[l - 1];
    std::vector<int> o, c0, c1;
    resize_axis(lv.w, sv.w, o, c0, c1);
    for (int d = 0; d < lv.w; d++) {
        int s = o[d], a0 = c0[d], a1 = c1[d];
        if (s < 0) { s = 0; a0 = 2048; a1 = 0; }              // fx = 0, sx = 0
        if (s >= sv.w - 1) { s = sv.w - 1; a0 = 2048; a1 = 0; } // fx = 0, sx = w-1
        xt.push_back(make_int2(s, a0 | (a1 << 16)));
    }
    // interior dword groups read their source columns as one 8-byte window: sx non-decreasing, span <= 8 bytes
    bool window_ok = true;
    for (int d = 0; d + 3 < lv.w; d += 4) {
        const int2 *g = &xt[lv.xtab + d];
        for (int k = 1; k < 4; ++k) window_ok = window_ok && g[k].x >= g[k - 1].x;
        window_ok = window_ok && g[3].x + 1 - g[0].x <= 7;
    }
    // the last group of a width that is no multiple of 4 is filled up with copies of the last entry (k_pyr_resize reads whole groups;
    // the bytes past w - 1 are replaced by border bytes): non-decreasing like the others, and no wider than a whole group
    const int2 xlast = xt[lv.xtab + lv.w - 1];
    for (int d = lv.w; d & 3; ++d) xt.push_back(xlast);
    const bool last_ok = (lv.w & 3) == 0 || xt[lv.xtab + lv.w - 1].x + 1 - xt[lv.xtab + (lv.w & ~3)].x <= 7;
    ex->resize_nxi[l] = window_ok ? 1 : 0;   // the 8-byte-window fast path may serve this level's interior groups
    // the copy rule of k_pyr_resize: borders are single mirror images of pixels of the same wave; k_pyr_resize_small otherwise
    ex->resize_copy[l] = window_ok && last_ok && lv.w >= EDGE + 1 && lv.h >= EDGE + 1 && resize_pairs_in_wave(lv.w) ? 1 : 0;
    {   // k_pyr_resize_small may use windows too (border dwords: reflected columns; row padding: clamped ones) if every dword
        // of the padded row keeps its four source columns within 7 bytes
        bool ok = true;
        for (int xw = (PADX - EDGE) >> 2; xw <= (PADX + lv.w + EDGE - 1) >> 2; ++xw) {
            int lo = 1 << 30, hi = -1;
            for (int b = 0; b < 4; ++b) {
                const int px = xw * 4 - PADX + b;
                const int sx = xt[lv.xtab + reflect101(px < -EDGE ? -EDGE : px > lv.w + EDGE - 1 ? lv.w + EDGE - 1 : px, lv.w)].x;
                lo = sx < lo ? sx : lo; hi = sx > hi ? sx : hi;
            }
            ok = ok && hi - lo <= 6;
        }
        ex->resize_tailwin[l] = ok ? 1 : 0;
    }
    resize_axis(lv.h, sv.h, o, c0, c1);
    for (int d = 0; d < lv.h; d++) {
        const int s = o[d];
        const int s0 = s < 0 ? 0 : (s < sv.h ? s : sv.h - 1);
        const int s1 = s + 1 < 0 ? 0 : (s + 1 < sv.h ? s + 1 : sv.h - 1);
        yt.push_back(make_int4(s0, s1, c0[d], c1[d]));
    }
    return ORBX_OK;
}

// The pyramid chain in one launch (k_pyr_chain): tiles and their rectangles per level.  Leaves chain_tiles = 0 (the per-level launches
// serve every batch) where the chain's conditions do not hold; never an error.
int plan_chain(orbx_extractor *ex, const std::vector<int2> &xt, const std::vector<int4> &yt)
{
    const int nl = ex->nlevels;
    ex->chain.clear(); ex->chain_tiles = 0; ex->chain_ldsA = ex->chain_ldsB = 0;
    bool ok = nl >= 2 && nl <= MAXL;
    for (int l = 1; l < nl && ok; ++l) ok = ex->resize_nxi[l] != 0 && ex->lv[l].w >= 8 && ex->lv[l].h >= 8;   // the 8-byte source window must hold at every level
    if (!ok) return ORBX_OK;
    const LevelInfo &l1 = ex->lv[1];
    // tiles of 48 x 36 px at level 1 (15 x 11 of them on 640 x 480): one frame's launch 22.3 us; 96 x 72: 26.8, 32 x 36: 22.6 -- a
    // workgroup's seven dependent levels are the floor, not the tile's area (ORBX_CHAIN_TW / _TH: development knobs)
    const int ctw = getenv("ORBX_CHAIN_TW") ? std::max(16, atoi(getenv("ORBX_CHAIN_TW"))) : 48, cth = getenv("ORBX_CHAIN_TH") ? std::max(16, atoi(getenv("ORBX_CHAIN_TH"))) : 36;
    const int nx = std::max(1, (l1.w + 2 * EDGE + ctw - 1) / ctw), ny = std::max(1, (l1.h + 2 * EDGE + cth - 1) / cth);
    int maxA = 0, maxB = 0;
    for (int j = 0; j < ny && ok; ++j)
        for (int i = 0; i < nx && ok; ++i) {
            ChainTile T;
            memset(&T, 0, sizeof(T));
            int ax0 = 0, ax1 = -1, ay0 = 0, ay1 = -1;        // what the deeper level reads of this one (inner coordinates, inclusive; empty: ax1 < ax0)
            for (int l = nl - 1; l >= 0; --l) {
                const LevelInfo &lv = ex->lv[l];
                int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1;
                ChainRect &rc = T.r[l];
                if (l >= 1) {
                    // ownership follows the INNER image: tile i owns the columns [w i / nx, w (i + 1) / nx) (cut at multiples of 4, so
                    // that the cuts are dword boundaries of the padded row), the first and last tile the 19-px border beside them --
                    // the tiles of all levels then cover the same part of the scene and a level's rectangle is little more than what
                    // the tile owns of it
                    const int xlo = (PADX - EDGE) >> 2, xhi = (PADX + lv.w + EDGE - 1) >> 2, R = lv.h + 2 * EDGE;
                    const auto bx = [&](int k) { return (int)((long long)k * lv.w / nx) & ~3; };
                    const auto by = [&](int k) { return (int)((long long)k * lv.h / ny); };
                    rc.oxw0 = (short)(i == 0 ? xlo : (PADX + bx(i)) >> 2); rc.oxw1 = (short)(i == nx - 1 ? xhi + 1 : (PADX + bx(i + 1)) >> 2);
                    rc.or0 = (short)(j == 0 ? 0 : EDGE + by(j)); rc.or1 = (short)(j == ny - 1 ? R : EDGE + by(j + 1));
                    for (int px = rc.oxw0 * 4 - PADX; px < rc.oxw1 * 4 - PADX; ++px) {
                        if (px < -EDGE || px >= lv.w + EDGE) continue;
                        const int x = reflect101(px, lv.w);
                        x0 = std::min(x0, x); x1 = std::max(x1, x);
                    }
                    for (int row = rc.or0; row < rc.or1; ++row) {
                        const int y = reflect101(row - EDGE, lv.h);
                        y0 = std::min(y0, y); y1 = std::max(y1, y);
                    }
                    if (x1 < x0 || y1 < y0) { x0 = y0 = 1 << 30; x1 = y1 = -1; rc.oxw1 = rc.oxw0; rc.or1 = rc.or0; }   // owns nothing here
                }
                if (ax1 >= ax0) { x0 = std::min(x0, ax0); x1 = std::max(x1, ax1); y0 = std::min(y0, ay0); y1 = std::max(y1, ay1); }
                if (x1 < x0) { x0 = x1 = 0; y0 = y1 = 0; }      // nothing owned, nothing needed below: a 1 x 1 rectangle keeps the kernel uniform
                x0 &= ~3;
                rc.nx0 = (short)x0; rc.ny0 = (short)y0; rc.nw = (short)(x1 - x0 + 1); rc.nh = (short)(y1 - y0 + 1);
                if (rc.nw > 1024 || rc.nh > 4096) ok = false;
                const int bytes = (((rc.nw + 15) & ~15) + 16) * rc.nh + 16;
                if (l & 1) maxB = std::max(maxB, bytes); else maxA = std::max(maxA, bytes);
                if (l >= 1) {      // what computing this rectangle reads of level l - 1
                    const int2 *xtab = &xt[lv.xtab];
                    const int4 *ytab = &yt[lv.ytab];
                    const int wsrc = ex->lv[l - 1].w;
                    ax0 = xtab[x0].x; ax1 = std::min(xtab[std::min(x1, lv.w - 1)].x + 1, wsrc - 1);
                    ay0 = std::min(ytab[y0].x, ytab[y0].y); ay1 = std::max(ytab[y1].x, ytab[y1].y);
                }
            }
            ex->chain.push_back(T);
        }
    maxA = (maxA + 15) & ~15; maxB = (maxB + 15) & ~15;
    // the coefficient tables of every tile as one block of 16-byte units: per level the rows, then per level the columns
    int maxT = 0;
    ex->chain_tabs.clear(); ex->chain_span.clear();
    for (const ChainTile &T : ex->chain) {
        const size_t first = ex->chain_tabs.size();
        std::vector<int2> rows;
        for (int l = 1; l < nl; ++l)
            for (int r = 0; r < T.r[l].nh; ++r) {
                const int4 y = yt[ex->lv[l].ytab + T.r[l].ny0 + r];
                const int s0 = y.x - T.r[l - 1].ny0, s1 = y.y - T.r[l - 1].ny0;
                if (s0 < 0 || s1 < s0 || s1 > 65535 || y.z < 0 || y.z > 65535 || y.w < 0 || y.w > 65535) ok = false;
                rows.push_back(make_int2(s0 | (s1 << 16), y.z | (y.w << 16)));
            }
        if (rows.size() & 1) rows.push_back(make_int2(0, 0));
        for (size_t k = 0; k < rows.size(); k += 2)
            ex->chain_tabs.push_back(make_uint4((unsigned)rows[k].x, (unsigned)rows[k].y, (unsigned)rows[k + 1].x, (unsigned)rows[k + 1].y));
        std::vector<int2> cols;
        for (int l = 1; l < nl; ++l)
            for (int c = 0; c < ((T.r[l].nw + 3) & ~3); ++c) {
                int2 x = xt[ex->lv[l].xtab + std::min(T.r[l].nx0 + c, ex->lv[l].w - 1)];     // (columns past the level: junk nobody reads)
                x.x -= T.r[l - 1].nx0;
                cols.push_back(x);
            }
        for (size_t k = 0; k < cols.size(); k += 2)      // (rounded-up widths are multiples of 4: an even count)
            ex->chain_tabs.push_back(make_uint4((unsigned)cols[k].x, (unsigned)cols[k].y, (unsigned)cols[k + 1].x, (unsigned)cols[k + 1].y));
        ex->chain_span.push_back(make_int2((int)first, (int)(ex->chain_tabs.size() - first)));
        maxT = std::max(maxT, (int)(ex->chain_tabs.size() - first) * 16);
    }
    if (ok && maxA + maxB + maxT <= 64 * 1024) { ex->chain_tiles = nx * ny; ex->chain_ldsA = maxA; ex->chain_ldsB = maxB; ex->chain_ldsT = maxT; }
    else ex->chain.clear();
    return ORBX_OK;
}

int prepare_chain(orbx_extractor *ex)
{
    if (ex->chain_tiles && ex->chain_ldsA + ex->chain_ldsB + ex->chain_ldsT > 48 * 1024)
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pyr_chain), hipFuncAttributeMaxDynamicSharedMemorySize, ex->chain_ldsA + ex->chain_ldsB + ex->chain_ldsT));
    return ORBX_OK;
}

void launch_level0(orbx_extractor *ex, const uint8_t *d_img, int stride, size_t frame_stride, int batch, hipStream_t st)
{
    const LevelInfo &l0 = ex->lv[0];
    const int aligned = (((uintptr_t)d_img | (uintptr_t)stride | (uintptr_t)frame_stride) & 3) == 0;
    ex->prof.start(0, st);
    // the linear form splits a piece index p into (row, piece) with the reciprocal inv = ceil(2^32 / d): exact while
    // p (inv d - 2^32) < 2^32 for every p < rows d -- holds with room for any size orbx_reserve accepts (sides <= 4,000 px:
    // 2 M x 500), checked here all the same so that a larger limit one day cannot shift pixels by a row unnoticed
    auto recip_exact = [](uint64_t count, uint64_t d) {
        const uint64_t inv = (0x100000000ull + d - 1) / d;
        return count == 0 || (count - 1) * (inv * d - 0x100000000ull) < 0x100000000ull;
    };
    const int rows = l0.h + 2 * EDGE, pp = l0.w / 8, nleft = PADX / 4 - ((PADX - EDGE) >> 2);
    const int nb = nleft + ((PADX + l0.w + EDGE - 1) >> 2) - ((PADX + l0.w) >> 2) + 1;
    if (aligned && l0.w % 8 == 0 && l0.w >= 64 && recip_exact((uint64_t)rows * pp, (uint64_t)pp) && recip_exact((uint64_t)rows * nb, (uint64_t)nb)) {
        const int nblk_int = (rows * pp + 255) / 256, nblk_b = (rows * nb + 63) / 64;
        hipLaunchKernelGGL(k_pyr_level0_lin, dim3(nblk_int + nblk_b, batch), dim3(64), 0, st, d_img, stride, frame_stride, ex->d_pyr,
                           ex->frame_bytes, l0, pp, (unsigned)((0x100000000ull + pp - 1) / pp), nblk_int, nb,
                           (unsigned)((0x100000000ull + nb - 1) / nb), nleft);
    } else {
        dim3 g((l0.stride / 4 + 63) / 64, (l0.h + 2 * EDGE + PYR_ROWS - 1) / PYR_ROWS, batch);
        hipLaunchKernelGGL(k_pyr_level0, g, dim3(64), 0, st, d_img, stride, frame_stride, ex->d_pyr, ex->frame_bytes, l0, aligned);
    }
    ex->prof.stop(0, st);
}

void launch_pyramid(orbx_extractor *ex, int batch, hipStream_t st)
{
    const int nl = ex->nlevels;
    orbx::KernelProfiler &pf = ex->prof;
    // Small batches -- the live tracker's one frame per call, a camera rig's few -- take the levels 1.. in ONE launch (k_pyr_chain): seven dependent launches of
    // a few microseconds each are 52 of one frame's 134 us of kernels.  Large batches keep the per-level launches (the one-launch form was
    // slower in the pipelined 64-frame step, profiles/r04_notes.md).  ORBX_PYR_CHAIN_MAX_BATCH moves the limit (0: never; tests run both).
    const char *cmb = getenv("ORBX_PYR_CHAIN_MAX_BATCH");            // (read per call: the tests flip it)
    const int chain_max_batch = cmb ? atoi(cmb) : 6;   // (tools/small_batch_sweep.py: ahead up to 6 frames per call, level at 8, behind from 16)
    if (ex->chain_tiles > 0 && batch <= chain_max_batch) {
        pf.start(1, st);
        hipLaunchKernelGGL(k_pyr_chain, dim3(ex->chain_tiles, batch), dim3(256), ex->chain_ldsA + ex->chain_ldsB + ex->chain_ldsT + 2 * MAXL * 16, st, ex->d_pyr, ex->frame_bytes,
                           (const LevelInfo *)ex->d_lv, nl, (const ChainTile *)ex->d_chain, (const uint4 *)ex->d_chain_tabs, (const int2 *)ex->d_chain_span,
                           ex->chain_ldsA, ex->chain_ldsB);
        pf.stop(1, st);
        return;
    }
    for (int l = 1; l < nl; l++) {
        const LevelInfo &lv = ex->lv[l];
        pf.start(1, st);
        if (ex->resize_copy[l]) {
            // full waves across a row x row groups of the IMAGE rows (the border rows ride with the rows they mirror), and the tiles
            int nfull, tws, dtile;
            resize_split(lv.w, nfull, tws, dtile);
            const int nrg = (lv.h + PYR_ROWS - 1) / PYR_ROWS;
            const int ntile = tws ? (nrg + (64 >> tws) - 1) / (64 >> tws) : 0;
            // row groups per full wave: two when one would need a second generation of resident waves (the kernel holds 8 waves
            // per SIMD) -- a second generation costs a whole wave's life, a longer wave only its extra rows.  Measured per 64-frame
            // chain of seven launches (round 4): 1 -> 0.100, 2 -> 0.094, 3 -> 0.098, 4 -> 0.103 ms
            int rpw = 1;
            while (rpw < 2 && (size_t)(nfull * ((nrg + rpw - 1) / rpw) + ntile) * batch > (size_t)ex->resident_waves) ++rpw;
            hipLaunchKernelGGL(k_pyr_resize, dim3(nfull * ((nrg + rpw - 1) / rpw) + ntile, batch), dim3(64), 0, st, ex->d_pyr, ex->frame_bytes,
                               ex->lv[l - 1], lv, ex->d_xt + lv.xtab, ex->d_yt + lv.ytab, nfull, tws, dtile, rpw);
        } else {
            const int ndw = ((PADX + lv.w + EDGE - 1) >> 2) - ((PADX - EDGE) >> 2) + 1;   // dwords of a padded row that hold border or image bytes
            const int tw_shift = ndw <= 16 ? 4 : ndw <= 32 ? 5 : 6;                      // tile: 16 x 4, 32 x 2 or 64 x 1 (dwords x row groups)
            const int nrg = (lv.h + 2 * EDGE + PYR_ROWS - 1) / PYR_ROWS, rpt = 64 >> tw_shift;
            const int ntw = (ndw + (1 << tw_shift) - 1) >> tw_shift;                     // tiles across a row (> 1 only when ndw > 64)
            hipLaunchKernelGGL(k_pyr_resize_small, dim3(ntw * ((nrg + rpt - 1) / rpt), batch), dim3(64), 0, st, ex->d_pyr, ex->frame_bytes,
                               ex->lv[l - 1], lv, ex->d_xt + lv.xtab, ex->d_yt + lv.ytab, ndw, tw_shift, ntw, ex->resize_tailwin[l]);
        }
        pf.stop(1, st);
    }
}

} // namespace orbx_detail
