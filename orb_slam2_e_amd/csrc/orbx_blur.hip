// orbx_blur.hip -- GaussianBlur 7x7 sigma 2 of every pyramid level (ORBextractor.cc:1093-1094) on the i8 matrix cores: k_blur,
// in the two tap-sum variants.  The host side below it lists the tile strips (plan_blur), builds and uploads the Toeplitz operand
// fragments (prepare_blur) and picks the variant and the accumulator seed (launch_blur).
#include "orbx_extract_internal.h"

using namespace orbx_detail;

namespace {

// GaussianBlur(7x7, sigma 2, REFLECT_101) in 8.8 fixed point: horizontal 7 taps exact in
// u16, vertical 7 taps exact in u32, min((v + 2^15) >> 16, 255).  The padded pyramid already holds the
// reflected border, so no index clamping.
//
// Both passes are products with a banded Toeplitz matrix of the taps, in exact integers on the i8 matrix
// cores (v_mfma_i32_32x32x32_i8): one wave blurs one 32 x 32 input tile,
//   H''[y'][x] = sum_k (P[y'][k] - 128) T[k - x - 1] + 128          (A = pixel rows as loaded, B = Toeplitz)
//   V^T[x][y]  = sum_y' H[y'][x] T[y' - y]                            (A = the accumulator of the first product)
// H'' fits 16 signed bits for tap sums up to 257 and goes into the second product as two i8 planes
// (H'' >> 8 and (H'' & 255) - 128, eight v_perm_b32 + xor per 16 values); the constant terms of both offsets
// ride in the accumulator seeds.  The first result has its column on the lane and its rows in the lane's 16
// registers, which is exactly an A (or B) operand of the next MFMA -- no LDS, no lane movement -- and since a
// dot product pairs operand bytes by position, the Toeplitz fragments (a 2-KB table built on the host) are
// simply written in the order in which the lane holds its rows; the hardware's K order never enters.  Taking
// the accumulator as A transposes the result: a lane ends with 16 x-consecutive outputs of ONE row, four per
// dword store.  A tile yields 24 x 26 valid outputs (7 taps of support inside 32 inputs, dword-aligned in x).
constexpr int BLUR_TW = 24, BLUR_TH = 26;
typedef int blur_v4i __attribute__((ext_vector_type(4)));
typedef int blur_v16i __attribute__((ext_vector_type(16)));
// A wave blurs a strip of BLUR_TPW x-adjacent tiles (96 x 26 outputs) and stages it in LDS, so that the rows
// leave as 16-byte pieces of 96 contiguous bytes instead of 4-byte pieces in 32 different lines.
constexpr int BLUR_TPW = 4, BLUR_SW = BLUR_TPW * BLUR_TW, BLUR_LROW = 112;   // strip width; LDS row stride (7 x 16 B)
constexpr int BLUR_IROW = 144;                                                 // LDS row stride of the 128-byte input window
// WIDE: tap sum 257 (blur_variant 1): H' = sum (P - 128) T needs a +128 bias to fit 16 signed bits, and the
// result can exceed 255.  Otherwise the first product starts from 0 and nothing saturates.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_blur(const uint8_t *__restrict__ pyr, uint8_t *__restrict__ blur,
                                              size_t frame_bytes, size_t blur_frame_bytes, const LevelInfo *__restrict__ L,
                                              const BlurTile *__restrict__ tiles, int ntiles,
                                              const uint4 *__restrict__ frag, int seed2)
{
    __shared__ __align__(16) uint8_t stage[4][BLUR_TH * BLUR_LROW];
    __shared__ __align__(16) uint8_t win[4][32 * BLUR_IROW];
    int f, wg;
    xcd_frame_item(f, wg);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ti = wg * 4 + wave;
    if (ti >= ntiles) return;
    const int r = lane & 31, h = lane >> 5;
    blur_v16i c1, c2, z;
#pragma unroll
    for (int g = 0; g < 16; ++g) { c1[g] = WIDE ? 128 : 0; c2[g] = seed2; z[g] = 0; }
    const BlurTile bt = tiles[ti];   // wave-uniform index: a scalar load
    struct { int w, h, stride; } lv = {bt.w, bt.h, bt.stride};
    const size_t base = (size_t)f * frame_bytes + bt.off + PADX;
    // the Toeplitz fragments (per-lane constants) are requested HERE, beside the window: left to the compiler they sank below the
    // window's LDS stores, a memory round trip of their own in front of the first MFMA
    uint4 f1 = frag[2 * lane], f2 = frag[2 * lane + 1];
    uint8_t *const st = stage[wave], *const wn = win[wave];
    // input window: rows y0-3 .. y0+28, columns x0-16 .. x0+111 as 8 aligned 16-byte pieces per row (whole 128-byte
    // lines per row instead of 32 bytes of 32 different lines per load).  Rows past the padded level and pieces past
    // the padded row are clamped: they only reach outputs that are not stored.
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const int i = lane + 64 * s4, row = i >> 3, pc = i & 7;
        const int yin = min(bt.y0 - 3 + row, lv.h + EDGE - 1), xo = min(PADX + bt.x0 - 16 + 16 * pc, lv.stride - 16);
        *reinterpret_cast<uint4 *>(wn + row * BLUR_IROW + 16 * pc) =
            *reinterpret_cast<const uint4 *>(pyr + (base - PADX) + (uint32_t)(__mul24(yin + EDGE, lv.stride) + xo));   // (24-bit factors: a full-rate multiply)
    }
    asm volatile("" : "+v"(f1.x), "+v"(f1.y), "+v"(f1.z), "+v"(f1.w), "+v"(f2.x), "+v"(f2.y), "+v"(f2.z), "+v"(f2.w));   // pins the loads above this point
    const blur_v4i b1 = {(int)f1.x, (int)f1.y, (int)f1.z, (int)f1.w}, b2 = {(int)f2.x, (int)f2.y, (int)f2.z, (int)f2.w};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < BLUR_TPW; ++k) {
        const int x0 = bt.x0 + BLUR_TW * k;
        if (x0 >= lv.w) break;
        // tile k: input columns x0-4 .. x0+27 = window bytes 12 + 24k ..; this lane's 16 of them
        const uint32_t *q = reinterpret_cast<const uint32_t *>(wn + r * BLUR_IROW + 12 + BLUR_TW * k + 16 * h);
        const uint4 p = make_uint4(q[0], q[1], q[2], q[3]);
        const blur_v4i a1 = {(int)(p.x ^ 0x80808080u), (int)(p.y ^ 0x80808080u), (int)(p.z ^ 0x80808080u), (int)(p.w ^ 0x80808080u)};
        const blur_v16i H = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, c1, 0, 0, 0);
        blur_v4i ah, al;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            // [b0(g), b0(g+1), b1(g), b1(g+1)] of two registers, then the low / high byte planes of four
            const uint32_t t01 = __builtin_amdgcn_perm((uint32_t)H[4 * d + 1], (uint32_t)H[4 * d], 0x05010400u);
            const uint32_t t23 = __builtin_amdgcn_perm((uint32_t)H[4 * d + 3], (uint32_t)H[4 * d + 2], 0x05010400u);
            al[d] = (int)(__builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u);
            ah[d] = (int)__builtin_amdgcn_perm(t23, t01, 0x07060302u);
        }
        const blur_v16i VL = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, b2, c2, 0, 0, 0);
        const blur_v16i VH = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, b2, z, 0, 0, 0);
        // lane = output row r; registers 4q .. 4q+3 = columns 8q + 4h + (0..3) of the tile
        if (r < BLUR_TH) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                uint32_t o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = ((uint32_t)VH[4 * q + e] << 8) + (uint32_t)VL[4 * q + e];   // v + 2^15: the result is byte 2
                    if (WIDE) o[e] = o[e] < 0x00ffffffu ? o[e] : 0x00ffffffu;
                }
                *reinterpret_cast<uint32_t *>(st + r * BLUR_LROW + BLUR_TW * k + 8 * q + 4 * h) =
                    __builtin_amdgcn_perm(o[1], o[0], 0x0c0c0602u) | __builtin_amdgcn_perm(o[3], o[2], 0x06020c0cu);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // rows out as 16-byte pieces, 6 per row, into the strip layout (orbx_internal.h): piece c of a row is one row of strip
    // (PADX + x) / 16 -- a lane's piece and the pieces of the rows above and below it in the same strip are contiguous
    uint8_t *const bdst = blur + (size_t)f * blur_frame_bytes + bt.boff;
#pragma unroll
    for (int s = 0; s < (BLUR_TH * (BLUR_SW / 16) + 63) / 64; ++s) {
        const int i = lane + 64 * s, c = i / BLUR_TH, row = i - c * BLUR_TH;   // rows fastest: four neighbouring lanes = 64 contiguous bytes of a strip
        const int x = bt.x0 + 16 * c, y = bt.y0 + row;
        if (c < BLUR_SW / 16 && y < lv.h && x < lv.w)
            *reinterpret_cast<uint4 *>(bdst + (uint32_t)(__mul24((PADX + x) >> 4, bt.bcol) + (y + EDGE) * 16)) =
                *reinterpret_cast<const uint4 *>(st + mul_u24((uint32_t)row, BLUR_LROW) + 16 * c);
    }
}

// (Measured in round 3 and dropped: k_octree and k_blur as ONE launch -- both follow k_fast_cells / the pyramid and precede k_describe,
// neither needs the other.  66-68 us for the pair instead of 54 + 27 alone, bit-exact, and the pipelined step 3 % SLOWER: the fused
// kernel allocates the octree's 121 VGPRs and 30 KB of LDS for every blur workgroup too.  Even the refactoring that made the two
// bodies callable from one kernel -- arguments through structs, the blur's LDS as a dynamic block -- cost the step 5.5 % with every
// kernel's own time unchanged (0.2737 against 0.2587 ms, three A/B rounds on one box, tools/ab.sh): with static LDS the compiler
// knows k_blur's occupancy limit and schedules for it.  What a kernel pins while it runs is what the other contexts pay for.)

} // namespace

namespace orbx_detail {

// Level l's tile strips: BLUR_SW x BLUR_TH outputs each, one wave's work.
int plan_blur(orbx_extractor *ex, int l)
{
    const LevelInfo &lv = ex->lv[l];
    for (int y0 = 0; y0 < lv.h; y0 += BLUR_TH)
        for (int x0 = 0; x0 < lv.w; x0 += BLUR_SW) {
            BlurTile t; t.x0 = (short)x0; t.y0 = (short)y0; t.w = (short)lv.w; t.h = (short)lv.h; t.off = lv.off; t.stride = lv.stride;
            t.boff = ex->boff[l]; t.bcol = ex->bcol[l]; t.pad[0] = t.pad[1] = 0;
            ex->tiles.push_back(t);
        }
    return ORBX_OK;
}

int prepare_blur(orbx_extractor *ex)
{
    // Toeplitz fragments of k_blur, per lane (r = lane & 31, h = lane >> 5), byte j of the 16-byte operand:
    // first product: input column 16h + j feeds output column r with tap (16h + j) - r - 1;
    // second product: the lane's j-th row is rho = (j & 3) + 8 (j >> 2) + 4h and feeds output row r with tap rho - r
    const int T[7] = {ex->taps[0], ex->taps[1], ex->taps[2], ex->taps[3], ex->taps[2], ex->taps[1], ex->taps[0]};
    uint8_t fr[64][2][16];
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 16; ++j) {
            const int r = lane & 31, h = lane >> 5, d1 = 16 * h + j - r - 1, d2 = (j & 3) + 8 * (j >> 2) + 4 * h - r;
            fr[lane][0][j] = (uint8_t)(d1 >= 0 && d1 < 7 ? T[d1] : 0);
            fr[lane][1][j] = (uint8_t)(d2 >= 0 && d2 < 7 ? T[d2] : 0);
        }
    ORBX_HIP(hipMalloc(&ex->d_blur_frag, sizeof(fr)));
    ORBX_HIP(hipMemcpyAsync(ex->d_blur_frag, fr, sizeof(fr), hipMemcpyHostToDevice, ex->stream));
    ORBX_HIP(hipStreamSynchronize(ex->stream));   // fr lives in this scope
    return ORBX_OK;
}

void launch_blur(orbx_extractor *ex, int batch, hipStream_t st)
{
    ex->prof.start(4, st);
    // with H'' = sum (P - 128) T + bias = 256 hi + lo' + 128:  H = H'' - bias + 128 S, so
    // V + 2^15 = 256 sum(T hi) + sum(T lo') + S (128 - bias + 128 S) + 2^15     (S = tap sum, bias = 128 iff S > 256)
    const int S = 2 * (ex->taps[0] + ex->taps[1] + ex->taps[2]) + ex->taps[3], nt = (int)ex->tiles.size();
#define ORBX_BLUR_LAUNCH(WIDE_, SEED_) hipLaunchKernelGGL(k_blur<WIDE_>, dim3((unsigned)((nt + 3) / 4), batch), dim3(256), 0, st, ex->d_pyr, ex->d_blur, \
        ex->frame_bytes, ex->blur_frame_bytes, ex->d_lv, ex->d_tiles, nt, ex->d_blur_frag, (SEED_))
    if (S > 256) ORBX_BLUR_LAUNCH(true, 128 * S * S + 32768);
    else ORBX_BLUR_LAUNCH(false, S * (128 + 128 * S) + 32768);
#undef ORBX_BLUR_LAUNCH
    ex->prof.stop(4, st);
}

} // namespace orbx_detail
