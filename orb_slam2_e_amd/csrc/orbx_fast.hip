// orbx_fast.hip -- FAST-9/16 per 30-px cell with non-max suppression and the threshold fallback (ComputeKeyPointsOctTree's cell
// loop, ORBextractor.cc:789-837): k_fast_cells, one wave per cell.  The host side below it sizes the kernel's LDS regions and picks
// the instantiation from the widest cell of the grid that plan_frame lays out (plan_fast, launch_fast).
#include <string.h>

#include <algorithm>

#include "orbx_extract_internal.h"

using namespace orbx_detail;

ORBX_PHASE_UNIT(fast)

namespace {

// --------------------------------------------------------------------- FAST
// Circle pixels p_k, k = 0..15: the 16-pixel Bresenham circle of radius 3 in OpenCV's makeOffsets order, starting at
// (0, 3) and running through (3, 0), (0, -3), (-3, 0).
// Necessary condition for a 9-arc (OpenCV's opposite-pair pre-test): a 9-arc contains
// one pixel of every opposite pair (k, k+8), so with d_k = v - p_k a dark arc needs
// min_k max(d_k, d_k+8) > th and a bright one max_k min(d_k, d_k+8) < -th (both at
// once cannot be a corner: a 9-arc holds both pixels of one pair).
// Evaluated for 4 horizontally adjacent pixels per lane, on packed u16 pairs
// (v_perm_b32 / v_pk_min_u16 / v_pk_max_u16; there is no byte-wise min/max).  With
// d_k = v - p_k:  min_k max(d_k, d_k+8) > th  <=>  v > max_k min(p_k, p_k+8) + th  (dark)
//                max_k min(d_k, d_k+8) < -th <=>  min_k max(p_k, p_k+8) > v + th  (bright)
// so the differences are never formed.  p = dword-aligned address of the 4 centre pixels
// in the LDS tile; the 7 rows x 12 bytes around it are read as dwords and the circle
// pixels of lanes-pixels (0,2) / (1,3) are pulled out as (even, odd) u16 pairs.
// Returns one byte per pixel: 1 = dark arc possible, 2 = bright, 0 = neither.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 pk2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t pk1(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
template <int DX>
__device__ __forceinline__ void fast_pick(const uint32_t r[3], u16x2 &E, u16x2 &O)
{
    constexpr int s = 4 + DX;                  // byte of pixel 0 in the 12-byte window r[0] | r[1] | r[2]
    constexpr int base = (DX < 0) ? s : s - 4; // ... inside the 8-byte pair handed to v_perm
    const uint32_t hi = (DX < 0) ? r[1] : r[2], lo = (DX < 0) ? r[0] : r[1];
    constexpr uint32_t selE = base | 0x0c00u | ((base + 2) << 16) | 0x0c000000u;       // {b, 0, b+2, 0}
    constexpr uint32_t selO = (base + 1) | 0x0c00u | ((base + 3) << 16) | 0x0c000000u; // {b+1, 0, b+3, 0}
    E = pk2(__builtin_amdgcn_perm(hi, lo, selE));
    O = pk2(__builtin_amdgcn_perm(hi, lo, selO));
}
// Both u16 halves: a > b ? 1 : 0, as v_pk_sub_u16 with clamp + v_pk_min_u16.  Written in asm because the compiler
// rewrites min(sub_sat(a, b), 1) into two 16-bit compares, two selects and a v_perm (six instructions instead of two);
// the operands come from VALU instructions, so there is no software-visible hazard to pad.
__device__ __forceinline__ uint32_t pk_gt01(uint32_t a, uint32_t b)
{
    uint32_t d;
    asm("v_pk_sub_u16 %0, %1, %2 clamp\n\tv_pk_min_u16 %0, %0, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(0x00010001u));
    return d;
}
// number of set bits of a wave mask below this lane
__device__ __forceinline__ int mask_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// PAIRS: bit k = opposite pair (k, k+8) takes part.  Returns bytes 0..3 = pixels 0..3: dark possible | bright possible << 1
// over the chosen pairs.  With all eight pairs both bits at once cannot be a corner (see above); with a subset either
// polarity is still open, so the codes of two subsets are ANDed first and the rule applied to the result
// (fast_resolve).  Rows whose pairs are not chosen are never loaded (the loads fold away at compile time).
template <int TS, unsigned PAIRS>
__device__ __forceinline__ uint32_t fast_pretest4(const uint8_t *p, uint32_t th2)
{
    uint32_t r[7][3];
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p + dy * TS);
        r[dy + 3][0] = q[-1]; r[dy + 3][1] = q[0]; r[dy + 3][2] = q[1];
    }
    u16x2 aE, aO, bE, bO, loE, loO, hiE, hiO;
    constexpr int FIRSTK = __builtin_ctz(PAIRS);
#define ORBX_PAIR(K, DYA, DXA)                                                                       \
    if constexpr ((PAIRS >> (K)) & 1u) {                                                             \
        fast_pick<DXA>(r[3 + (DYA)], aE, aO);                                                        \
        fast_pick<-(DXA)>(r[3 - (DYA)], bE, bO);                                                     \
        if constexpr ((K) == FIRSTK) {                                                               \
            loE = __builtin_elementwise_min(aE, bE); loO = __builtin_elementwise_min(aO, bO);        \
            hiE = __builtin_elementwise_max(aE, bE); hiO = __builtin_elementwise_max(aO, bO);        \
        } else {                                                                                     \
            loE = __builtin_elementwise_max(loE, __builtin_elementwise_min(aE, bE));                 \
            loO = __builtin_elementwise_max(loO, __builtin_elementwise_min(aO, bO));                 \
            hiE = __builtin_elementwise_min(hiE, __builtin_elementwise_max(aE, bE));                 \
            hiO = __builtin_elementwise_min(hiO, __builtin_elementwise_max(aO, bO));                 \
        }                                                                                            \
    }
    ORBX_PAIR(0, 3, 0)   // circle pixels 0 / 8
    ORBX_PAIR(1, 3, 1)   // 1 / 9
    ORBX_PAIR(2, 2, 2)   // 2 / 10
    ORBX_PAIR(3, 1, 3)   // 3 / 11
    ORBX_PAIR(4, 0, 3)   // 4 / 12
    ORBX_PAIR(5, -1, 3)  // 5 / 13
    ORBX_PAIR(6, -2, 2)  // 6 / 14
    ORBX_PAIR(7, -3, 1)  // 7 / 15
#undef ORBX_PAIR
    u16x2 vE, vO;
    fast_pick<0>(r[3], vE, vO);
    const u16x2 t = pk2(th2);
    // per half "a > b" as 0 / 1: saturating difference clamped to 1
    const uint32_t dE = pk_gt01(pk1(vE), pk1(loE + t)), dO = pk_gt01(pk1(vO), pk1(loO + t));
    const uint32_t gE = pk_gt01(pk1(hiE), pk1(vE + t)), gO = pk_gt01(pk1(hiO), pk1(vO + t));
    return (dE | (gE << 1)) | ((dO | (gO << 1)) << 8);
}
// dark and bright both possible over all eight pairs cannot be a corner -> 0
__device__ __forceinline__ uint32_t fast_resolve(uint32_t code) { return code & ~((code & (code >> 1) & 0x01010101u) * 3u); }
constexpr unsigned FAST_PAIRS_A = 0x11u;   // compass pairs 0/8 and 4/12 on every pixel; the other six on what is left, pixel by pixel

// cornerScore<16>: (largest arc-minimum of e_k over the 16 circular 9-arcs) - 1
// where e = d (dark) or -d (bright), d_k = v - p_k; it is a corner at threshold th iff that
// arc-minimum exceeds th, and the score does not depend on th.
// Computed on packed halves.  X[k] (k = 0..7) holds e_k in its low and e_(k+8) in its high 16 bits, every value
// biased to 0x4100 + e: the bit patterns 0x4001..0x41ff are positive normal f16 numbers, and for those the float order IS
// the integer order -- so gfx950's three-operand packed v_pk_minimum3_f16 / v_pk_maximum3_f16 serve as integer min3 /
// max3 on two values at once (no NaN, no zero, no denormal among the operands; nothing is rounded: min / max only
// select).  X[k+8] is X[k] with its halves swapped, which the op_sel modifiers do for free.  min over the 9-arc
// starting at k = min3 of three 3-arcs; 16 + 4 instructions instead of 64.  Returns max_k min(e_k .. e_(k+8)) + 0x4100.
template <int S1, int S2> __device__ __forceinline__ uint32_t pk_min3_h(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    if constexpr (S1 && S2) asm("v_pk_minimum3_f16 %0, %1, %2, %3 op_sel:[0,1,1] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    else if constexpr (S2) asm("v_pk_minimum3_f16 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    else asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ uint32_t pk_max3_h(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ uint32_t fast_arc_best_packed(const uint32_t X[8])
{
    uint32_t m3[8], m9[8];
    m3[0] = pk_min3_h<0, 0>(X[0], X[1], X[2]); m3[1] = pk_min3_h<0, 0>(X[1], X[2], X[3]);
    m3[2] = pk_min3_h<0, 0>(X[2], X[3], X[4]); m3[3] = pk_min3_h<0, 0>(X[3], X[4], X[5]);
    m3[4] = pk_min3_h<0, 0>(X[4], X[5], X[6]); m3[5] = pk_min3_h<0, 0>(X[5], X[6], X[7]);
    m3[6] = pk_min3_h<0, 1>(X[6], X[7], X[0]); m3[7] = pk_min3_h<1, 1>(X[7], X[0], X[1]);
    m9[0] = pk_min3_h<0, 0>(m3[0], m3[3], m3[6]); m9[1] = pk_min3_h<0, 0>(m3[1], m3[4], m3[7]);
    m9[2] = pk_min3_h<0, 1>(m3[2], m3[5], m3[0]); m9[3] = pk_min3_h<0, 1>(m3[3], m3[6], m3[1]);
    m9[4] = pk_min3_h<0, 1>(m3[4], m3[7], m3[2]); m9[5] = pk_min3_h<1, 1>(m3[5], m3[0], m3[3]);
    m9[6] = pk_min3_h<1, 1>(m3[6], m3[1], m3[4]); m9[7] = pk_min3_h<1, 1>(m3[7], m3[2], m3[5]);
    const uint32_t a = pk_max3_h(m9[0], m9[1], m9[2]), b = pk_max3_h(m9[3], m9[4], m9[5]);
    const uint32_t c = pk_max3_h(m9[6], m9[7], a), m = pk_max3_h(b, c, c);
    return max(m & 0xffffu, m >> 16);
}

// One wave per 30-px cell (ORBextractor.cc:789-837): cv::FAST(cell, iniThFAST, nms=true),
// rerun with minThFAST only if the cell came back empty; candidates are written
// in FAST raster order, coordinates relative to (minBorderX, minBorderY).
// Packed candidate: y<<20 | x<<8 | score.
//
// Phases: (1) cell tile -> LDS, loaded as 16-byte pieces, four lanes to a tile row; then, as the reference does, one pass at iniThFAST and -- only if that
// pass emits nothing (a wave-uniform branch; on textured frames almost every cell has a corner at iniThFAST) -- a
// second one at minThFAST:
// (2a) every pixel, 4 adjacent pixels per lane on packed u16: the opposite-pair pre-test on the two compass
// pairs only (0/8 and 4/12: the vertical pair needs no byte shuffling across dwords); the 4-pixel groups that still
// hold a possible corner (18 % of them at level 0, 67 % at level 7 on the synthetic frames) are compacted in raster
// order into an LDS group queue; (2b) the queued groups' live pixels go to the pixel queue, and the other six pairs are tested
// with a lane per pixel (a group-wise test on packed halves worked on all four pixels of a group of which one or two were
// alive), survivors (4 % ... 28 % of the pixels) compacted in place; (3) survivors only: arc score -> score map (0 below
// the pass's threshold, which is all the non-max test needs: a neighbour that is no corner at this threshold scores
// less than any corner); (4) 3x3 strict NMS and ordered emission, one loop.
// TS / SS (tile and score-map strides) are compile-time so that the 16 circle
// offsets fold into ds_read immediates.
template <int TS, int SS>
__global__ __launch_bounds__(64) void k_fast_cells(const uint8_t *__restrict__ pyr, size_t frame_bytes,
                                                   const LevelInfo *__restrict__ L,
                                                   const CellInfo *__restrict__ cells, int *__restrict__ cell_count,
                                                   int cells_per_frame, uint32_t *__restrict__ cands,
                                                   size_t cands_per_frame, int iniTh, int minTh,
                                                   int tile_bytes, int sc_bytes, int queue_bytes)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint8_t *tile = smem;
    // LDS per wave decides how many waves a CU holds (the kernel speeds up with occupancy well beyond 20 waves per CU, and what
    // it leaves free is what the other pipeline contexts' kernels can use): the group queue is dead once stage (2b) has read
    // it and the score map is born after that, so they share one region (sc_bytes = the larger of the two)
    uint8_t *sc = smem + tile_bytes;
    uint32_t *gqueue = reinterpret_cast<uint32_t *>(smem + tile_bytes);
    unsigned short *queue = reinterpret_cast<unsigned short *>(smem + tile_bytes + sc_bytes);
    (void)queue_bytes;
    int c, f;
    xcd_frame_item(f, c);
    c = cells_per_frame - 1 - c;   // dispatch order: the small levels' cells (most survivors, longest waves) first, level 0 last -- a shorter tail
    const int lane = threadIdx.x;
    ORBX_PH_INIT(0);
    const FastCell ci = cells[c];   // everything the wave needs about its cell: no second dependent table read
    const int cw = ci.cw, ch = ci.ch, zw = cw - 6, zh = ch - 6;
    int total = 0;
    if (zw > 0 && zh > 0) {
        // (1) tile: pixel (x, y) of the cell lives at tile[y*TS + 5 + x], so that zone pixel 0 (cell pixel 3) sits
        // on the dword boundary at column 8 whatever the cell's position: the pre-test's 4-pixel groups then cover a
        // zone row with ceil(zw/4) groups.  The row's ndw dwords come over as 16-byte PIECES at byte addresses (see
        // load_u128_unaligned), LP lanes side by side on a tile row -- four where a row is at most 64 bytes -- and 64 / LP
        // rows per instruction: a lane's piece never changes.  Three load instructions per cell instead of eleven dword
        // loads, and 4.2 % fewer vector instructions in the kernel.  What the pieces do NOT save are texture-addresser
        // accesses ("quads and spans"): a 16-byte lane counts like four dword lanes, 1.23 accesses at an
        // arbitrary byte address, 227 per wave against 209 before (profiles/vmem_pieces_notes.md).  All
        // loads of a chunk of NB instructions are issued before the first is stored, and none of them sits behind a
        // branch (a lane without work reads the cell's last row / the row's last piece again): the wave spends ONE memory
        // latency here, not one per step -- this phase was 44 % of a wave's life when every load was followed by its
        // store.  48 rows = one chunk of three instructions covers every cell of a 640 x 480 frame.  The last piece of a
        // row reads up to 12 bytes past the dwords the pre-test needs: plan_fast proves for every cell that they lie inside
        // the level's padded row.  The stores know no branch either: the lane that read a row or a piece again stores it
        // again (same bytes to the same place), and a piece goes into the tile whole -- what lies past the row's ndw dwords
        // are image bytes where nothing was written before, in columns whose pixels stage (2b) masks -- except that the
        // fourth piece of a 52-byte row (TS = 52 is no multiple of 16, hence dword stores) ends with its first dword.
        // The wait for the chunk's loads is ONE, in front of the stores: the compiler otherwise moves a load whose
        // value only a predicated store takes behind that store's branch.  (Several cells per wave with the next cell's
        // tile in flight during the current one's work: kernel 3-20 % slower, the tail grows; dropped.)
        constexpr int LP = TS > 64 ? 8 : 4, RPI = 64 / LP, NB = TS == 52 ? 3 : TS == 64 ? 4 : 6;
        static_assert(TS % 16 == 0 || TS == 52, "a row takes whole pieces, or three and a dword");
        const int npc = fast_row_pieces(cw);
        const uint8_t *img = pyr + (size_t)f * frame_bytes + ci.img_off;
        {
            const int xp = min(lane & (LP - 1), npc - 1), yr = lane / LP;
            for (int yb = 0; yb < ch; yb += NB * RPI) {
                uint4 v[NB];
                uint32_t *d[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int y = min(yb + yr + i * RPI, ch - 1);
                    v[i] = load_u128_unaligned(img + ((uint32_t)__mul24(y, ci.stride) + 16u * (uint32_t)xp));
                    d[i] = reinterpret_cast<uint32_t *>(tile + __mul24(y, TS) + 16 * xp);
                }
#pragma unroll
                for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i].z), "+v"(v[i].w));
#pragma unroll
                for (int i = 0; i < NB; ++i) d[i][0] = v[i].x;
                if (TS != 52 || xp < 3) {
#pragma unroll
                    for (int i = 0; i < NB; ++i) { d[i][1] = v[i].y; d[i][2] = v[i].z; d[i][3] = v[i].w; }
                }
            }
        }
        __syncthreads();
        ORBX_PH(0, lane == 0);   // tile load
        constexpr int zc0 = 8;                        // tile column of zone pixel 0
        const uint8_t *t0 = tile + 3 * TS + zc0;      // zone pixel (0,0)
        const unsigned long long lt = (1ull << lane) - 1ull;
        const int g0 = zc0 >> 2, ngx = ci.ngx, ngrp = ngx * zh;
        const int qstep = ci.qstep, rstep = ci.rstep;         // lane + 64 -> (gx + rstep, y + qstep), one carry
        unsigned short *const dump = queue + zw * zh;         // one spare slot per lane for rejected pixels
        uint32_t *out = cands + (size_t)f * cands_per_frame + ci.cand_off;
        for (int pass = 0; pass < 2; ++pass) {
            const int th = pass ? minTh : iniTh;
            const uint32_t th2 = (uint32_t)th | ((uint32_t)th << 16);
            // (2a) compass pairs on every group; group queue entry = code | y << 2 | gx << 10 (the code uses bits 0-1 of
            // every byte).  A group = the 4 pixels of one tile dword; groups overlapping the zone row, in raster order.
            int ngq = 0;
            {
                int y = (lane * ci.inv_ngx) >> 16, gx = lane - y * ngx;
                for (int p0 = 0; p0 < ngrp; p0 += 64) {
                    uint32_t code = 0;
                    // a row's last group may reach past the zone: those pixels are masked in (2b), on the queued groups only
                    if (p0 + lane < ngrp) code = fast_pretest4<TS, FAST_PAIRS_A>(tile + __mul24(y + 3, TS) + 4 * (g0 + gx), th2);
                    const unsigned long long b = __ballot(code != 0);
                    if (code) gqueue[ngq + mask_rank(b)] = code | ((uint32_t)y << 2) | ((uint32_t)gx << 10);
                    ngq += __popcll(b);
                    gx += rstep; y += qstep;
                    if (gx >= ngx) { gx -= ngx; ++y; }
                }
            }
            __syncthreads();
            ORBX_PH(1, lane == 0);   // stage A
            // (2b) the other six pairs, per PIXEL: of a queued group's four pixels one or two are still alive, and a lane that tests a
            // whole group on packed halves works on all four (151 instructions per 64 groups against 61 + 45 per 64 pixels).
            // First the queued groups' alive pixels (compass code != 0, inside the zone) go to the pixel queue in raster order, entry
            // y<<6 | x | compass code<<12 ...
            int np = 0;
            for (int q0 = 0; q0 < ngq; q0 += 64) {
                uint32_t code = 0;
                int ent = 0;
                if (q0 + lane < ngq) {
                    const uint32_t e = gqueue[q0 + lane];
                    const int y = (e >> 2) & 63, gx = (e >> 10) & 63;
                    ent = (y << 6) + 4 * gx;                                                   // zone x of the group's pixel 0
                    code = e & 0x03030303u & (0xffffffffu >> (8 * max(0, 4 * gx + 4 - zw)));   // pixels at zone x >= zw are outside
                }
                if (__ballot(code != 0)) {
                    // alive pixels of this lane: bytes 0..3 are 0..3 -> one bit per pixel, n = how many
                    const uint32_t nz = (code | (code >> 1)) & 0x01010101u;
                    const int n = __popc(nz);
                    const unsigned long long c0 = __ballot(n & 1), c1 = __ballot(n & 2), c2 = __ballot(n & 4);
                    int pos = np + mask_rank(c0) + 2 * mask_rank(c1) + 4 * mask_rank(c2);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { // branch-free: dead pixels go to the lane's dump slot
                        const int ac = (code >> (8 * j)) & 3;
                        unsigned short *dst = ac ? queue + pos : dump + lane;
                        *dst = (unsigned short)((ent + j) | (ac << 12));
                        pos += ac != 0;
                    }
                    np += __popcll(c0) + 2 * __popcll(c1) + 4 * __popcll(c2);
                }
            }
            // ... then a lane per pixel: max over the six pairs of min(p_k, p_k+8) and min of their max, the two threshold tests, ANDed with
            // the compass code; both polarities possible over all eight pairs cannot be a corner.  Survivors are compacted IN PLACE
            // (entry y<<6 | x | polarity<<12): a write lands at or below the position its lane read in this round, and the wave reads
            // before it writes.
            int nq = 0;
            for (int q0 = 0; q0 < np; q0 += 64) {
                int pol = 0, ent = 0;
                if (q0 + lane < np) {
                    const int e = queue[q0 + lane], x = e & 63, y = (e >> 6) & 63, ac = e >> 12;
                    ent = e & 0xfff;
                    const uint8_t *t = t0 + y * TS + x;
                    const int v = t[0];
                    const int a1 = t[3 * TS + 1], b1 = t[-3 * TS - 1], a2 = t[2 * TS + 2], b2 = t[-2 * TS - 2], a3 = t[TS + 3], b3 = t[-TS - 3];
                    const int a5 = t[-TS + 3], b5 = t[TS - 3], a6 = t[-2 * TS + 2], b6 = t[2 * TS - 2], a7 = t[-3 * TS + 1], b7 = t[3 * TS - 1];
                    const int lo = max(max(max(min(a1, b1), min(a2, b2)), min(a3, b3)), max(max(min(a5, b5), min(a6, b6)), min(a7, b7)));
                    const int hi = min(min(min(max(a1, b1), max(a2, b2)), max(a3, b3)), min(min(max(a5, b5), max(a6, b6)), max(a7, b7)));
                    const bool dark = (ac & 1) && v > lo + th, bright = (ac & 2) && hi > v + th;
                    pol = dark == bright ? 0 : dark ? 1 : 2;
                }
                const unsigned long long bm = __ballot(pol != 0);
                if (pol) queue[nq + mask_rank(bm)] = (unsigned short)(ent | (pol << 12));
                nq += __popcll(bm);
            }
            __syncthreads();
            ORBX_PH(2, lane == 0);   // stage B
            // the score map takes over the group queue's region: all zero, then (3) writes the survivors' scores
            for (int i = lane; i < ((zh + 2) * SS + 3) / 4; i += 64) reinterpret_cast<uint32_t *>(sc)[i] = 0;
            __syncthreads();
            // (3) arc score of the survivors
            for (int q0 = 0; q0 < nq; q0 += 64) {
                if (q0 + lane < nq) {
                    const int e = queue[q0 + lane], x = e & 63, y = (e >> 6) & 63;
                    // e_k = v - p_k (dark) or p_k - v (bright) = (p_k ^ m) - (v ^ m) with m = 0xff / 0; pairs (k, k+8) packed
                    // and biased in one xor-add each: halves (p ^ m) + (0x4100 - (v ^ m)) lie in 0x4001..0x41ff, no carry
                    const uint8_t *t = t0 + y * TS + x;
                    const uint32_t m1 = (e >> 12) == 1 ? 0xffu : 0u, m2 = m1 | (m1 << 16);
                    const uint32_t c1 = 0x4100u - ((uint32_t)t[0] ^ m1), c2 = c1 | (c1 << 16);
                    uint32_t X[8];
                    X[0] = (((uint32_t)t[3 * TS] | ((uint32_t)t[-3 * TS] << 16)) ^ m2) + c2;
                    X[1] = (((uint32_t)t[3 * TS + 1] | ((uint32_t)t[-3 * TS - 1] << 16)) ^ m2) + c2;
                    X[2] = (((uint32_t)t[2 * TS + 2] | ((uint32_t)t[-2 * TS - 2] << 16)) ^ m2) + c2;
                    X[3] = (((uint32_t)t[TS + 3] | ((uint32_t)t[-TS - 3] << 16)) ^ m2) + c2;
                    X[4] = (((uint32_t)t[3] | ((uint32_t)t[-3] << 16)) ^ m2) + c2;
                    X[5] = (((uint32_t)t[-TS + 3] | ((uint32_t)t[TS - 3] << 16)) ^ m2) + c2;
                    X[6] = (((uint32_t)t[-2 * TS + 2] | ((uint32_t)t[2 * TS - 2] << 16)) ^ m2) + c2;
                    X[7] = (((uint32_t)t[-3 * TS + 1] | ((uint32_t)t[3 * TS - 1] << 16)) ^ m2) + c2;
                    const int best = (int)fast_arc_best_packed(X) - 0x4100;
                    sc[(y + 1) * SS + x + 1] = (uint8_t)(best > th ? best - 1 : 0);
                }
            }
            __syncthreads();
            ORBX_PH(3, lane == 0);   // zero + arc score
            // (4) 3x3 strict non-max suppression on the survivors and (5) emission in queue (= raster) order, pass by pass of 64
            for (int q0 = 0; q0 < nq; q0 += 64) {
                bool ismax = false;
                uint32_t word = 0;
                if (q0 + lane < nq) {
                    const int e = queue[q0 + lane], x = e & 63, y = (e >> 6) & 63;
                    const uint8_t *q = sc + (y + 1) * SS + x + 1;
                    const int s = q[0];
                    // strictly above all eight neighbours (scores are >= 0, so this also says s > 0); no short-circuit
                    // branches: eight LDS bytes, three v_max3, one compare
                    const int m = max(max(max(q[-1], q[1]), max(q[-SS - 1], q[-SS])), max(max(q[-SS + 1], q[SS - 1]), max(q[SS], q[SS + 1])));
                    ismax = s > m;
                    word = ((uint32_t)(ci.dy + y + 3) << 20) | ((uint32_t)(ci.dx + x + 3) << 8) | (uint32_t)s;
                }
                const unsigned long long b = __ballot(ismax);
                const int pos = total + __popcll(b & lt);
                if (ismax && pos < ci.cap) out[pos] = word;
                total += __popcll(b);
            }
            ORBX_PH(4, lane == 0);   // NMS + emission
            if (total > 0 || minTh == iniTh) break; // empty at iniThFAST: once more at minThFAST (:820-824)
            __syncthreads();                        // the queues are rewritten
        }
    }
    if (lane == 0) cell_count[(size_t)f * cells_per_frame + c] = total;
    ORBX_PH(5, lane == 0);       // epilogue
    ORBX_PH(6, lane == 0);       // (count of waves x timer cost)
    ORBX_PH_END(lane == 0);
}

} // namespace

namespace orbx_detail {

// Tile and score-map strides, LDS regions.  maxcw x maxch: the largest cell (CellInfo::cw / ch) of the frame's grid.
int plan_fast(orbx_extractor *ex, int maxcw, int maxch)
{
    // tile row = 5 spare bytes + the cell + the packed pre-test's right-hand dword; zone <= 63 (6-bit queue
    // coordinates)
    if (maxcw + 12 > 80 || maxch > 69) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "FAST cell larger than the LDS tile");
    // three instantiations by the widest cell: tile stride 52 / score-map stride 40 for cells up to 44 px (zone <= 38: its
    // ten 4-pixel groups end at tile column 51 and its score row, with the two border columns, at 39) -- the 36-43 px
    // cells of every usual image size; 64 / 64; 80 / 80.  LDS per wave sets how many waves a CU holds.
    ex->TS = maxcw <= 44 ? 52 : (maxcw + 12 <= 64) ? 64 : 80;
    ex->SS = maxcw <= 44 ? 40 : ex->TS;
    ex->tile_bytes = (ex->TS * maxch + 15) & ~15;
    const int gq_bytes = 4 * (((maxcw - 6 + 3) >> 2) * (maxch - 6));                               // group queue
    ex->sc_bytes = (std::max(ex->SS * (maxch - 6 + 2), gq_bytes) + 15) & ~15;                      // score map, sharing the group queue's region
    ex->queue_bytes = (2 * (maxcw - 6) * (maxch - 6) + 2 * 64 + 15) & ~15;                         // pixel queue + the pre-test's dump slots
    ex->fast_lds = ex->tile_bytes + ex->sc_bytes + ex->queue_bytes;
    // The tile load's 16-byte pieces: piece p < fast_row_pieces(cw) of cell row y < ch covers bytes [16 p, 16 p + 16) from
    // img_off + y stride, i.e. columns PADX + x0 - 5 + 16 p ... of padded row y0 + EDGE + y.  By the grid (x0 >= MIN_BORDER,
    // x0 + cw <= w - 16, 4 ndw <= cw + 8, 16 npc <= 4 ndw + 12) the last byte read is at most column PADX + w - 2 of row
    // h + 2 -- inside the inner image, the last cell of the last level included, and frames lie frame_bytes apart, so the
    // last frame reads nothing behind the allocation.  Checked cell by cell all the same: a grid that breaks it is refused.
    for (const CellInfo &c : ex->cells) {
        if (c.cw <= 6 || c.ch <= 6) continue;   // no zone: the kernel loads nothing
        const LevelInfo &lv = ex->lv[c.level];
        const int col0 = PADX + c.x0 - 5, col1 = col0 + 16 * fast_row_pieces(c.cw), row0 = c.y0 + EDGE, row1 = row0 + c.ch;
        const bool in_row = col0 >= 0 && col1 <= lv.stride && row0 >= 0 && row1 <= lv.h + 2 * EDGE;
        const bool at_cell = c.img_off == lv.off + row0 * lv.stride + col0 && c.stride == lv.stride;
        if (!in_row || !at_cell || (size_t)lv.off + (size_t)lv.stride * (lv.h + 2 * EDGE) > ex->frame_bytes)
            ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "FAST tile pieces would read outside the level's padded rows");
    }
    return ORBX_OK;
}

int debug_fast_pieces(const orbx_extractor *ex, int32_t *out, int cap, int *n)
{
    *n = (int)ex->cells.size();
    if (*n > cap) ORBX_FAIL(ORBX_ERR_CAPACITY, "cell buffer too small");
    for (const CellInfo &c : ex->cells) {
        const bool loads = c.cw > 6 && c.ch > 6;
        const int32_t rec[8] = {c.level, c.img_off, c.stride, loads ? c.ch : 0, loads ? fast_row_pieces(c.cw) : 0, c.cw, c.x0, c.y0};
        memcpy(out, rec, sizeof(rec));
        out += 8;
    }
    return ORBX_OK;
}

void launch_fast(orbx_extractor *ex, int batch, hipStream_t st)
{
    // (profiled: the kernel's own start and end through hipExtLaunchKernelGGL -- see KernelProfiler::pair)
    hipEvent_t e0, e1;
    ex->prof.pair(2, &e0, &e1);
#define ORBX_FAST_LAUNCH(TS_, SS_) hipExtLaunchKernelGGL((k_fast_cells<TS_, SS_>), dim3(ex->cells_per_frame, batch), dim3(64), ex->fast_lds, st, e0, e1, 0, \
        (const uint8_t *)ex->d_pyr, ex->frame_bytes, (const LevelInfo *)ex->d_lv, (const CellInfo *)ex->d_cells, ex->d_cell_count, ex->cells_per_frame, ex->d_cands, \
        ex->cands_per_frame, ex->prm.ini_th_fast, ex->prm.min_th_fast, ex->tile_bytes, ex->sc_bytes, ex->queue_bytes)
    if (ex->TS == 52) ORBX_FAST_LAUNCH(52, 40);
    else if (ex->TS == 64) ORBX_FAST_LAUNCH(64, 64);
    else ORBX_FAST_LAUNCH(80, 80);
#undef ORBX_FAST_LAUNCH
}

} // namespace orbx_detail
