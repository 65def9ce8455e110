// orbx_describe.hip -- IC_Angle, steered BRIEF and the output records (ORBextractor.cc:77-147, :845-860, :1103-1111): k_describe,
// 16 keypoints per workgroup.  The host side below it: how many selected-keypoint slots a level has (level_slots -- the octree's
// worst case, which is also what sizes this kernel's grid) and the per-level constants and launch (launch_describe).
#include <string.h>

#include <algorithm>

#include "orbx_extract_internal.h"
#include "orbx_math.h"

using namespace orbx_detail;

ORBX_PHASE_UNIT(describe)

namespace {

__constant__ signed char c_pattern[1024] = {
#include "orb_pattern.inc"
};

// ----------------------------------------------------- orientation + rBRIEF
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v)
{
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}

// Sum over the wave, returned wave-uniform: four row_shr steps leave each 16-lane row's total in its last lane,
// row_bcast:15 / row_bcast:31 carry it across the rows into lane 63 (six DPP adds, no LDS traffic).
__device__ __forceinline__ int wave_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// N independent wave sums, step by step across all of them: a DPP instruction needs its source two VALU slots old, and
// with N chains interleaved those slots hold the other chains' steps instead of s_nop.
template <int N> __device__ __forceinline__ void wave_sum_n(int (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x111, 0xf, 0xf, true);   // row_shr:1
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x112, 0xf, 0xf, true);   // row_shr:2
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x114, 0xf, 0xf, true);   // row_shr:4
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x118, 0xf, 0xf, true);   // row_shr:8
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __builtin_amdgcn_update_dpp(0, v[i], 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_amdgcn_readlane(v[i], 63);
}

// 16 keypoints per 256-thread workgroup (4 per wave).  Phase 0: one lane per
// keypoint finds its level and pixel; phase 1: IC_Angle moments (:77-104) on the
// unblurred level, one wave per keypoint at a time; phase 2: one lane per
// keypoint evaluates fastAtan2 and the exact sin/cos ONCE (they are wave-uniform
// values -- evaluating them in every lane of a keypoint's wave would cost 64x the
// instructions); phase 3: computeOrbDescriptor (:108-147) on the blurred level
// and the output record (:845-855 octave/size, :1103-1109 pt *= scale).
// IC_Angle weights for v_dot4c_i32_i8: the 31x31 window is read as 31 rows x 8 dwords starting at (x-15, y-15); dword
// d = row*8 + w holds u = 4w-15 .. 4w-12 of row v = row - 15.  Inside the circular patch (|u| <= umax[|v|],
// ORBextractor.cc:454-469) the U weight of a byte is u and its V weight is v, outside both are 0.  The pixels enter as
// p - 128 (one xor with 0x80808080 makes them signed bytes): the patch is symmetric in u and in v, so the weights of all
// 248 dwords sum to zero and sum(u (p - 128)) = sum(u p) = m10 exactly, likewise m01 -- two accumulating dot products per
// dword and nothing else.
struct MomentWeights { uint32_t u[248], v[248]; };
constexpr MomentWeights make_moment_weights()
{
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    MomentWeights m{};
    for (int d = 0; d < 248; ++d) {
        const int v = d / 8 - 15, av = v < 0 ? -v : v;
        uint32_t wu = 0, wv = 0;
        for (int k = 0; k < 4; ++k) {
            const int u = 4 * (d % 8) + k - 15, au = u < 0 ? -u : u;
            if (au <= umax[av]) { wu |= (uint32_t)(u & 0xff) << (8 * k); wv |= (uint32_t)(v & 0xff) << (8 * k); }
        }
        m.u[d] = wu; m.v[d] = wv;
    }
    return m;
}
__device__ const MomentWeights c_momw = make_moment_weights();


constexpr int DESC_PD = 1;   // (DESC_KPB: orbx_extract_internal.h)
// Per-level constants of k_describe, passed by value (kernel-argument memory: scalar loads, nothing to wait for behind a
// table pointer).  Workgroup `item` of a frame serves chunk item - chunk_base[level] of the level with
// chunk_base[level] <= item < chunk_base[level + 1]: 16 consecutive entries of that level's selected-keypoint slots.
struct DescLevels {
    int off[MAXL], stride[MAXL], sel_base[MAXL], patch[MAXL], chunk_base[MAXL + 1];
    int boff[MAXL], bcol[MAXL];   // the level in the blurred buffer's strip layout
    float scale[MAXL];
};
__global__ __launch_bounds__(256) void k_describe(const uint8_t *__restrict__ pyr, const uint8_t *__restrict__ blur,
                                                  size_t frame_bytes, size_t blur_frame_bytes, const DescLevels D, int nlevels,
                                                  const uint32_t *__restrict__ sel_all, int sel_per_frame,
                                                  const int *__restrict__ level_count,
                                                  orbx_keypoint *__restrict__ kps, uint8_t *__restrict__ desc,
                                                  int *__restrict__ counts, int cap, int trig_variant, uint32_t *__restrict__ mirror, int mirror_desc)
{
    // mirror (one frame per call only): the caller's pinned result block {count, 12 bytes | kps[cap] | desc[cap][32]} as dwords, desc at
    // dword mirror_desc -- every record is stored there as well (posted writes), so that no copy kernel runs behind this one
    __shared__ uint32_t s_coff[DESC_KPB];   // patch centre, byte offset inside the frame's pyramid
    __shared__ int s_valid[DESC_KPB], s_out[DESC_KPB], s_m10[DESC_KPB], s_m01[DESC_KPB];
    __shared__ uint32_t s_pk[DESC_KPB];
    __shared__ uint32_t s_boff[DESC_KPB];   // blurred window: byte offset of (strip of its first aligned piece, first aligned row) in the frame's strips
    __shared__ int s_bx[DESC_KPB];          // bits 0-3 (x - 18) mod 16: bit 3 = which half of the strip the first piece is, bits 0-2 = shift inside it; bits 4-5: (y - 18) mod 4
    __shared__ float s_angle[DESC_KPB], s_cos[DESC_KPB], s_sin[DESC_KPB];
    __shared__ uint32_t s_patch[4][40 * 12 + 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    ORBX_PH_INIT(1);
    int f, item;
    xcd_frame_item(f, item);
    // the workgroup's level and chunk follow from its index alone, so the keypoint words and the level counts (which
    // only decide validity and the OUTPUT position) are read side by side: one memory latency, not two
    int level = 0;
    for (int l = 1; l < nlevels; ++l) level += item >= D.chunk_base[l];
    const int stride = D.stride[level];
    // the level counts of the frame: wave-uniform addresses, so they come through the scalar cache (as per-lane loads of
    // 16 lanes they were 8 of a workgroup's ~100 texture-addresser instructions)
    int first = 0, mine = 0, total = 0;
    {
        const int *lc = level_count + __builtin_amdgcn_readfirstlane(f) * nlevels;
        for (int l = 0; l < nlevels; ++l) {
            const int c = lc[l];
            first += l < level ? c : 0;
            mine = l == level ? c : mine;
            total += c;
        }
    }
    if (tid < DESC_KPB) {
        const int j = (item - D.chunk_base[level]) * DESC_KPB + tid;   // slot within the level
        const uint32_t pk = sel_all[(size_t)f * sel_per_frame + D.sel_base[level] + j];   // (slots past the level's count: never used)
        if (item == 0 && tid == 0) { counts[f] = total < cap ? total : cap; if (mirror) mirror[0] = (uint32_t)(total < cap ? total : cap); }
        const int x = (int)((pk >> 8) & 0xfffu) + MIN_BORDER, y = (int)(pk >> 20) + MIN_BORDER;
        s_valid[tid] = j < mine && first + j < cap;
        s_out[tid] = first + j;
        s_pk[tid] = pk;
        s_coff[tid] = (uint32_t)(D.off[level] + (y + EDGE) * stride + PADX + x);
        const int X = PADX + x - 18;                 // window origin in the padded row (>= PADX - 2)
        const int Y = y + EDGE - 18;                 // window's first row in the padded level
        s_boff[tid] = (uint32_t)(D.boff[level] + (X >> 4) * D.bcol[level] + (Y & ~3) * 16);
        s_bx[tid] = (X & 15) | ((Y & 3) << 4);
    }
    __syncthreads();
    ORBX_PH(8, tid == 0);    // keypoint lookup
    if (!s_valid[0]) return; // a level's slots fill from 0: nothing in this chunk
    const uint8_t *const fpyr = pyr + (size_t)f * frame_bytes, *const fblur = blur + (size_t)f * blur_frame_bytes;
    // IC_Angle (:77-104): every lane owns 4 dwords of the 31x31 window (fixed per lane, so are
    // their weights) and reads them straight from the unblurred level; two dot4 per dword.
    // No branches on "slot in use": an unused slot reads the window of slot 0 (in use, see above) and its results are
    // dropped, so the loads of all four keypoints of a wave are in flight together.
    uint32_t *patch = s_patch[wv];
    // The 37x37 blurred window of steered BRIEF (|offset| <= 18) is staged in LDS as 40 rows of 12 dwords: the 8-byte ALIGNED pieces
    // that cover columns x-18 .. x+18 (six per row; the window starts (x - 18) mod 8 bytes into the first), from the 4-ALIGNED row at
    // or above y-18.  Aligned pieces never straddle a strip of the blurred buffer, and in a strip consecutive rows are 16 bytes
    // apart: four lanes that take the same piece of four consecutive aligned rows read one 64-byte span -- the unit the texture
    // addresser works in -- so a wave-wide load is 16 of those instead of ~35 (row-major: the four lanes of a group sat in two rows).
    // Every lane owns four fixed pieces (piece d + 64 jj: row d % 40, column d / 40); which strip a column falls into depends on
    // whether the window starts in the first or the second half of its strip -- two offset sets per lane, chosen per keypoint by a
    // wave-uniform select.  The windows are loaded PD keypoints ahead of their use, the first ones together with the moment
    // windows: they depend on the keypoint's position only
    constexpr int PR = 18, PW = 12, PROWS = 40, PD = DESC_PD, NPL = 4; // patch radius; LDS row = 12 dwords; staged rows; prefetch distance; loads per lane
    const int bcol = D.bcol[level];
    uint32_t poffA[NPL], poffB[NPL]; int pslot[NPL];
#pragma unroll
    for (int jj = 0; jj < NPL; ++jj) {
        const int d = lane + 64 * jj, dd = min(d, PROWS * 6 - 1);   // pieces past the window repeat its last one
        const int col = dd / PROWS, row = dd - PROWS * col;
        poffA[jj] = (uint32_t)(row * 16 + __mul24((8 * col) >> 4, bcol) + ((8 * col) & 15));
        poffB[jj] = (uint32_t)(row * 16 + __mul24((8 + 8 * col) >> 4, bcol) + ((8 + 8 * col) & 15) - 8);   // (the base below already carries the 8)
        pslot[jj] = (int)mul_u24((uint32_t)row, PW) + 2 * col;
    }
    uint2 nxt[PD][NPL];
    auto load_patch = [&](int j, uint2 (&r)[NPL]) {   // unused slots read slot 0's window (no branch in front of a load)
        const int kp = wv * (DESC_KPB / 4) + j, kpv = s_valid[kp] ? kp : 0;
        const int bx = __builtin_amdgcn_readfirstlane(s_bx[kpv]);
        const uint8_t *win = fblur + (uint32_t)__builtin_amdgcn_readfirstlane((int)s_boff[kpv]) + (bx & 8);   // first aligned piece of row y-18
#pragma unroll
        for (int jj = 0; jj < NPL; ++jj) __builtin_memcpy(&r[jj], win + ((bx & 8) ? poffB[jj] : poffA[jj]), 8);
    };
    // IC_Angle window, 31 rows x 32 bytes from (x-15, y-15): lane d (+ 64 jj) owns the 8-byte piece d % 4 of row d / 4 (dwords
    // 2 (d % 4) and + 1 of that row): two 8-byte loads per keypoint instead of four dwords; pieces past row 30 re-read row 0 with
    // weights 0
    int wU[4], wV[4];
    uint32_t moff[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int d = lane + 64 * jj, row = d >> 2, piece = d & 3;
        const bool in = row < 31;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int w = in ? 8 * row + 2 * piece + k : 0;
            wU[2 * jj + k] = in ? (int)c_momw.u[w] : 0; wV[2 * jj + k] = in ? (int)c_momw.v[w] : 0;
        }
        moff[jj] = (uint32_t)(__mul24(in ? row : 0, stride) + 8 * piece);
    }
    {
        uint32_t px[DESC_KPB / 4][4];
#pragma unroll
        for (int j = 0; j < DESC_KPB / 4; ++j) {
            const int kp = wv * (DESC_KPB / 4) + j, kpv = s_valid[kp] ? kp : 0;
            // wave-uniform value read from LDS: tell the compiler, so the loads take a scalar base + 32-bit lane offset
            const uint8_t *win = fpyr + (uint32_t)__builtin_amdgcn_readfirstlane((int)s_coff[kpv]) - 15 - (ptrdiff_t)15 * stride; // (x-15, y-15)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) __builtin_memcpy(&px[j][2 * jj], win + moff[jj], 8);
        }
#pragma unroll
        for (int j = 0; j < PD; ++j) load_patch(j, nxt[j]);
        int mom[2 * (DESC_KPB / 4)];   // m10, m01 of the wave's four keypoints: eight independent sums
#pragma unroll
        for (int j = 0; j < DESC_KPB / 4; ++j) {
            int m10 = 0, m01 = 0;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int ps = (int)(px[j][jj] ^ 0x80808080u);
                m10 = __builtin_amdgcn_sdot4(ps, wU[jj], m10, false);
                m01 = __builtin_amdgcn_sdot4(ps, wV[jj], m01, false);
            }
            mom[2 * j] = m10; mom[2 * j + 1] = m01;
        }
        wave_sum_n<2 * (DESC_KPB / 4)>(mom);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < DESC_KPB / 4; ++j) { s_m10[wv * (DESC_KPB / 4) + j] = mom[2 * j]; s_m01[wv * (DESC_KPB / 4) + j] = mom[2 * j + 1]; }
        }
    }
    __syncthreads();
    ORBX_PH(9, tid == 0);    // moments
    if (tid < DESC_KPB && s_valid[tid]) {
        const float angle = orbx_fast_atan2((float)s_m01[tid], (float)s_m10[tid]);
        const float factorPI = (float)(3.14159265358979323846 / 180.f);
        float a, b;
        if (trig_variant == 0) orbx_sincos_glibc_f32(angle * factorPI, &b, &a); // a = cos, b = sin
        else orbx_sincos_f32(angle * factorPI, &b, &a);
        s_angle[tid] = angle; s_cos[tid] = a; s_sin[tid] = b;
    }
    __syncthreads();
    ORBX_PH(10, tid == 0);   // atan2 + sincos
    // steered BRIEF: lane i evaluates tests 4i..4i+3 of its wave's current keypoint, sampling the staged window.
    // Rotation on packed f32 (v_pk_mul_f32 / v_pk_add_f32, the same IEEE operations as the scalar form):
    // (x', y') = (px a - py b, px b + py a) = (px, px) * (a, b) + (-py, py) * (b, a); adding 1.5 * 2^23 rounds both to
    // the nearest-even integer (= cvRound) and leaves 0x4B400000 + value in the bits, which feed the address
    // multiply-add directly (its 24-bit multiplicand is 0x400000 + y').
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 PX[8], PY[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const signed char *pp = c_pattern + 16 * lane + 4 * t;
        PX[2 * t] = f32x2{(float)pp[0], (float)pp[0]}; PY[2 * t] = f32x2{-(float)pp[1], (float)pp[1]};
        PX[2 * t + 1] = f32x2{(float)pp[2], (float)pp[2]}; PY[2 * t + 1] = f32x2{-(float)pp[3], (float)pp[3]};
    }
    unsigned dacc = 0;   // lane 8j + m: dword m of the descriptor of the wave's keypoint j
#pragma unroll
    for (int j = 0; j < DESC_KPB / 4; ++j) {
        const int kp = wv * (DESC_KPB / 4) + j;
        const float a = s_cos[kp], b = s_sin[kp];
#pragma unroll
        for (int jj = 0; jj < NPL; ++jj) *reinterpret_cast<uint2 *>(patch + pslot[jj]) = nxt[j % PD][jj];
        if (j + PD < DESC_KPB / 4) load_patch(j + PD, nxt[j % PD]);
        if (!s_valid[kp]) continue;
        // patch centre, minus what the magic-number bits add: (0x400000 * 40 + 0x4B400000) mod 2^32
        const int bxs = __builtin_amdgcn_readfirstlane(s_bx[kp]);
        const uint8_t *pc = reinterpret_cast<const uint8_t *>(patch) + (PR + (bxs >> 4)) * (PW * 4) + PR + (bxs & 7);
        const f32x2 ab = {a, b}, ba = {b, a}, magic = {12582912.0f, 12582912.0f};
        unsigned nib = 0, tv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const f32x2 w = (PX[t] * ab + PY[t] * ba) + magic;
            const unsigned off = __umul24(__float_as_uint(w.y), PW * 4) + __float_as_uint(w.x) - (0x400000u * (PW * 4) + 0x4B400000u);
            tv[t] = pc[(int)off];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) nib |= (unsigned)(tv[2 * t] < tv[2 * t + 1]) << t;
        // lanes 8j .. 8j+7 hold the eight nibbles of dword j: DPP row_shl (lane i reads lane i+n of its 16-lane row)
        const unsigned byte = nib | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)nib, 0x101, 0xf, 0xf, true) << 4); // even lanes
        const unsigned w = byte | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)byte, 0x102, 0xf, 0xf, true) << 8) |
                           ((unsigned)__builtin_amdgcn_update_dpp(0, (int)byte, 0x104, 0xf, 0xf, true) << 16) |
                           ((unsigned)__builtin_amdgcn_update_dpp(0, (int)byte, 0x106, 0xf, 0xf, true) << 24);
        // lane 8m holds dword m of this keypoint's descriptor: hand it to lane 8j + m, where it waits for the wave's one store
        const unsigned wv_ = (unsigned)__shfl((int)w, 8 * (lane & 7));
        if ((lane >> 3) == j) dacc = wv_;
        ORBX_PH(11 + j, tid == 0);   // BRIEF of the wave's keypoint j (incl. waiting for its patch)
    }
    // Output records of the wave's four keypoints, which sit side by side in the frame's arrays (a level's slots fill from
    // 0, so the valid ones are a prefix): ONE store of 32 lanes x 4 bytes for the descriptors and ONE of 28 lanes x 4 bytes
    // for the keypoint structs (7 dwords each: x, y, size, angle, response, octave, class_id), instead of a store per
    // keypoint and per struct -- the stores go through the texture addresser like the loads, and the kernel is bound by it
    {
        const int kp0 = wv * (DESC_KPB / 4);
        const size_t o0 = (size_t)f * cap + s_out[kp0];
        if (lane < 32 && s_valid[kp0 + (lane >> 3)]) reinterpret_cast<uint32_t *>(desc + o0 * 32)[lane] = dacc;
        if (mirror && lane < 32 && s_valid[kp0 + (lane >> 3)]) mirror[mirror_desc + o0 * 8 + lane] = dacc;
        if (lane < 28) {
            const int jk = lane / 7, fld = lane - 7 * jk, kp = kp0 + jk;
            if (s_valid[kp]) {
                const uint32_t pk = s_pk[kp];
                float x = (float)((int)((pk >> 8) & 0xfffu) + MIN_BORDER), y = (float)((int)(pk >> 20) + MIN_BORDER);
                if (level != 0) { x *= D.scale[level]; y *= D.scale[level]; }   // :1103-1109
                const uint32_t val = fld == 0 ? __float_as_uint(x) : fld == 1 ? __float_as_uint(y) :
                                     fld == 2 ? __float_as_uint((float)D.patch[level]) : fld == 3 ? __float_as_uint(s_angle[kp]) :
                                     fld == 4 ? __float_as_uint((float)(pk & 0xffu)) : fld == 5 ? (uint32_t)level : 0xffffffffu;
                reinterpret_cast<uint32_t *>(kps + o0)[lane] = val;
                if (mirror) mirror[4 + o0 * 7 + lane] = val;
            }
        }
    }
    ORBX_PH(15, tid == 0);
    ORBX_PH_END(tid == 0);
}

} // namespace

namespace orbx_detail {

// slots of a level in the selected-keypoint array: DistributeOctTree's worst case (see orbx_create) + 1
int level_slots(const LevelInfo &lv) { return std::max(lv.N + 4, 4 * lv.nIni); }

void launch_describe(orbx_extractor *ex, int batch, hipStream_t st)
{
    const int nl = ex->nlevels;
    ex->prof.start(5, st);
    DescLevels D;
    memset(&D, 0, sizeof(D));
    int nchunks = 0;
    for (int l = 0; l < nl; l++) {
        const LevelInfo &lv = ex->lv[l];
        D.off[l] = lv.off; D.stride[l] = lv.stride; D.sel_base[l] = lv.sel_base; D.patch[l] = lv.patch; D.scale[l] = lv.scale;
        D.boff[l] = ex->boff[l]; D.bcol[l] = ex->bcol[l];
        D.chunk_base[l] = nchunks;
        nchunks += (level_slots(lv) + DESC_KPB - 1) / DESC_KPB;   // a level holds at most max(N + 3, 4 nIni) keypoints
    }
    for (int l = nl; l <= MAXL; l++) D.chunk_base[l] = nchunks;
    hipLaunchKernelGGL(k_describe, dim3(nchunks, batch), dim3(256), 0, st, ex->d_pyr, ex->d_blur, ex->frame_bytes, ex->blur_frame_bytes, D, nl,
                       ex->d_sel, ex->sel_per_frame, ex->d_level_count, ex->d_kps, ex->d_desc, ex->d_counts, ex->kcap, ex->prm.trig_variant,
                       batch == 1 ? ex->mirror : (uint32_t *)nullptr, ex->mirror_desc);
    ex->prof.stop(5, st);
}

} // namespace orbx_detail
