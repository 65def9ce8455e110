// orbm_frame.hip -- the frame the windowed searches read, for gfx950: Frame::AssignFeaturesToGrid on the host and on the device.
//   Frame::AssignFeaturesToGrid, Frame::PosInGrid             src/Frame.cc:245-260, :397-407
//   Frame::UndistortKeyPoints, Frame::ComputeImageBounds      :419-449, :451-479   (orbm_undistort.h)
//   the grid's cell pitch mfGridElementWidthInv / HeightInv   :95-96               (KeyFrame's copy: src/KeyFrame.cc:36,44)
//
// A search visits a window's keypoints in Frame::GetFeaturesInArea order (src/Frame.cc:342-395): column-major cells, insertion
// order inside a cell.  Sorted by (grid cell, index) the candidates of a window are a few contiguous runs of one array.  Here
//   1. sort_frame does that on the host for the entries that take a frame as host arrays (a SortedFrame travels with its call);
//   2. k_frame_build does it on the device, one workgroup per frame, for a frame that stays in HBM (orbm_frame): from host arrays
//      (orbm_frame_create) or straight from the extractor's device results, undistortion inside the build, one frame or a batch
//      in one launch (orbm_frame_from_extractor[_cam], orbm_frames_from_extractor);
//   3. the blocks of destroyed frames are recycled through a pool (a frame per image must not cost a hipMalloc); an alias
//      (orbm_frame_alias: the KeyFrame of a Frame) shares its block under a reference count.
// A frame-making call waits for its stream once (twice where the caller's arrays need the extractor's count first); the count of
// the last call is orbm_debug_last_frame_build_waits.  The searches take a frame through FrameSrc (orbm_search_internal.h).
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "common.h"
#include "orbm_internal.h"
#include "orbm_search_internal.h"
#include "orbm_undistort.h"
#include "orbx_internal.h"
#include "orbx_math.h"

using namespace orbm_detail;

namespace {

// A frame resident in HBM (orbm_frame): Frame::AssignFeaturesToGrid (src/Frame.cc:245-260, PosInGrid :397-407) on the device.
// ONE workgroup lays the keypoints out in (cell, index) order -- the order Frame::GetFeaturesInArea visits a window in --
//   1. cell of every keypoint (the reference's float arithmetic), cell histogram in LDS;
//   2. exclusive scan of the histogram = cell_off;
//   3. rank of a keypoint inside its cell = keypoints of the same cell with a smaller index: per 64-keypoint chunk the
//      lanes compare cells pairwise (all waves), then one wave walks the chunks in order with a running count per cell;
//   4. gather: position, level, right coordinate, angle, descriptor, permutation.
// Keypoints outside the grid (Frame::PosInGrid false: no window search ever returns them) follow the sorted part at positions
// ns .. n-1 in index order: the searches over explicit candidate lists (SearchByBoW) address features by index, grid or not.
// Keypoints come as cv::KeyPoint records (mvKeysUn; or the extractor's device results, optionally with the undistorted
// coordinates beside them), n from the host or from the extractor's count array.
constexpr int FB_T = 1024, FB_MAXN = SEQ_MAXN, FB_NC = FRAME_GRID_COLS * FRAME_GRID_ROWS;
constexpr size_t FB_LDS = sizeof(int) * (2 * (size_t)FB_NC + 2) + (size_t)FB_MAXN * (2 + 2 + 1 + 1);

// What k_frame_build reads of one frame: where the keypoints are (n on the device or from the host, never more than n_max) and the
// arrays of the block it fills.  res_hdr / res_perm: a second copy of the header and the permutation, in the launch's result block
// (the batch form: ONE copy brings every frame's pair to the host), or null.
struct FrameJob {
    const orbx_keypoint *kps; const uint4 *desc_raw; const float2 *xy_un; const float *uright_raw; const int *n_dev;
    int n_host, n_max;
    SeqKp *kp; uint4 *desc; float *angle; int *perm; int *cell_off; FrameHdr *hdr;
    FrameHdr *res_hdr; int *res_perm;
};

// One workgroup per frame.  BATCH: frame blockIdx.x of `table` (in the call's staged block); otherwise `one`, from the kernel's own
// arguments (chosen when compiled: a pointer that may be either makes every access of the record a per-lane flat load).  cam: the
// keypoint coordinates go through Frame::UndistortKeyPoints (undistort_point; cam.k1 == 0: they stay) unless xy_un replaces them.
template <bool BATCH>
__global__ __launch_bounds__(FB_T) void k_frame_build(FrameJob one, const FrameJob *__restrict__ table, GridParams gp, orbm_distortion cam)
{
    const FrameJob J = BATCH ? table[blockIdx.x] : one;
    const orbx_keypoint *__restrict__ kps = J.kps;
    const uint4 *__restrict__ desc_raw = J.desc_raw;
    const float2 *__restrict__ xy_un = J.xy_un;
    const float *__restrict__ uright_raw = J.uright_raw;
    const int *__restrict__ n_dev = J.n_dev;
    SeqKp *__restrict__ kp = J.kp;
    uint4 *__restrict__ desc = J.desc;
    float *__restrict__ angle = J.angle;
    int *__restrict__ perm = J.perm, *__restrict__ cell_off = J.cell_off, *__restrict__ res_perm = J.res_perm;
    FrameHdr *hdr = J.hdr, *res_hdr = J.res_hdr;
    extern __shared__ __align__(16) unsigned char fb_sm[];
    int *s_off = reinterpret_cast<int *>(fb_sm);                 // [FB_NC + 1] histogram, then exclusive scan
    int *s_run = s_off + FB_NC + 1;                              // [FB_NC + 1] keypoints of the cell placed so far (last entry: scan carry)
    unsigned short *s_cell = reinterpret_cast<unsigned short *>(s_run + FB_NC + 1);   // [n] cell or 0xffff
    unsigned short *s_pos = s_cell + FB_MAXN;                    // [n] sorted position
    unsigned char *s_low = reinterpret_cast<unsigned char *>(s_pos + FB_MAXN), *s_tot = s_low + FB_MAXN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(min(n_dev ? *n_dev : J.n_host, J.n_max), FB_MAXN);
    __shared__ int s_omin, s_omax;     // octave range of the keypoints (the searches index per-level tables with it)
    if (tid == 0) { s_omin = INT_MAX; s_omax = INT_MIN; }
    for (int c = tid; c <= FB_NC; c += FB_T) { s_off[c] = 0; s_run[c] = 0; }
    __syncthreads();
    for (int j = tid; j < n; j += FB_T) {
        float x, y;
        if (xy_un) { x = xy_un[j].x; y = xy_un[j].y; }
        else undistort_point(cam, kps[j].x, kps[j].y, &x, &y);
        const int px = orbx_f2i_x86(roundf((x - gp.min_x) * gp.inv_w)), py = orbx_f2i_x86(roundf((y - gp.min_y) * gp.inv_h));   // NaN: outside
        const bool in = !(px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS);
        const int c = in ? px * FRAME_GRID_ROWS + py : FB_NC;   // FB_NC: outside the grid -- kept behind the sorted part, in index order
        s_cell[j] = (unsigned short)c;
        if (in) atomicAdd(&s_off[c], 1);
    }
    __syncthreads();
    {   // exclusive scan of FB_NC counts: 3 per thread, wave scan, wave totals through s_run's spare slots
        constexpr int PER = FB_NC / FB_T;
        static_assert(FB_NC % FB_T == 0, "cells per thread");
        int v[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { v[k] = s_off[tid * PER + k]; sum += v[k]; }
        const int inc = orbx::wave_incl_scan(sum);
        __shared__ int wsum[FB_T / 64];
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        int run = base + inc - sum;
#pragma unroll
        for (int k = 0; k < PER; ++k) { s_off[tid * PER + k] = run; run += v[k]; }
        if (tid == FB_T - 1) s_off[FB_NC] = run;
    }
    __syncthreads();
    for (int c = tid; c <= FB_NC; c += FB_T) cell_off[c] = s_off[c];
    // rank inside the chunk: lanes of one cell, in lane order
    const int nchunk = (n + 63) / 64;
    for (int ch = wave; ch < nchunk; ch += FB_T / 64) {
        const int j = ch * 64 + lane;
        const int c = j < n ? (int)s_cell[j] : 0xffff;
        int low = 0, tot = 0;
#pragma unroll 8
        for (int l = 0; l < 64; ++l) {
            const int cl = __shfl(c, l);
            const int same = cl == c;
            tot += same;
            low += same && l < lane;
        }
        if (j < n) { s_low[j] = (unsigned char)low; s_tot[j] = (unsigned char)(tot - 1); }   // (tot - 1 <= 63 fits a byte)
    }
    __syncthreads();
    if (wave == 0) {        // chunks in index order: the running count of a cell is what the earlier chunks put there
        for (int ch = 0; ch < nchunk; ++ch) {
            const int j = ch * 64 + lane;
            const int c = j < n ? (int)s_cell[j] : 0xffff;
            int base = 0;
            if (c != 0xffff) base = s_run[c];
            if (c != 0xffff) {
                s_pos[j] = (unsigned short)(s_off[c] + base + s_low[j]);
                if (s_low[j] == s_tot[j]) s_run[c] = base + s_tot[j] + 1;    // the cell's last lane of the chunk
            }
        }
    }
    __syncthreads();
    int omin = INT_MAX, omax = INT_MIN;
    for (int j = tid; j < n; j += FB_T) {
        const int sp = s_pos[j];
        // every load in front of the first store (the pointers come from a table: the compiler cannot tell them apart, and a
        // load behind a store would wait for its own round trip)
        const orbx_keypoint k = kps[j];
        const uint4 d0 = desc_raw[2 * j], d1 = desc_raw[2 * j + 1];
        const float ur = uright_raw ? uright_raw[j] : -1.0f;
        const float2 c = xy_un ? xy_un[j] : make_float2(k.x, k.y);
        omin = min(omin, k.octave); omax = max(omax, k.octave);
        SeqKp o;
        if (xy_un) { o.x = c.x; o.y = c.y; }
        else undistort_point(cam, k.x, k.y, &o.x, &o.y);        // (a pure function of the keypoint: the bits of the first pass)
        o.uright = ur;
        o.octave = k.octave;
        kp[sp] = o; angle[sp] = k.angle; perm[sp] = j;
        if (res_perm) res_perm[sp] = j;
        desc[2 * sp] = d0; desc[2 * sp + 1] = d1;
    }
    if (omin <= omax) { atomicMin(&s_omin, omin); atomicMax(&s_omax, omax); }
    __syncthreads();
    if (tid == 0) {
        const FrameHdr h = {n, s_off[FB_NC], s_omin, s_omax};
        *hdr = h;
        if (res_hdr) *res_hdr = h;
    }
}

// Frame::UndistortKeyPoints on n points, one thread each (orbm_undistort_points)
__global__ __launch_bounds__(MT) void k_undistort_points(orbm_distortion cam, const float2 *__restrict__ xy, int n, float2 *__restrict__ xy_un)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= n) return;
    float2 o;
    undistort_point(cam, xy[i].x, xy[i].y, &o.x, &o.y);
    xy_un[i] = o;
}

// The grid of a frame with the given bounds: mfGridElementWidthInv / mfGridElementHeightInv (src/Frame.cc:95-96)
GridParams grid_params(float min_x, float min_y, float max_x, float max_y)
{
    return {min_x, min_y, (float)FRAME_GRID_COLS / (max_x - min_x), (float)FRAME_GRID_ROWS / (max_y - min_y)};
}

// order = grid cell << 16 | keypoint index: ascending order = the order in which
// Frame::GetFeaturesInArea (src/Frame.cc:342-395) lists its result (column-major cells,
// insertion order inside a cell); 0xffffffff = not in the grid / skipped.
struct WinKp { float x, y, uright; int octave; unsigned order; };

// Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:245-260,397-407), on the host: n float ops.
void build_winkp(const orbx_keypoint *kps, int n, const uint8_t *skip, const float *uright, const GridParams &gp, std::vector<WinKp> &wk)
{
    wk.resize(n ? n : 1);
    for (int j = 0; j < n; ++j) {
        const int px = orbx_f2i_x86(roundf((kps[j].x - gp.min_x) * gp.inv_w)), py = orbx_f2i_x86(roundf((kps[j].y - gp.min_y) * gp.inv_h));
        const bool in = !(px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS);
        wk[j].x = kps[j].x; wk[j].y = kps[j].y; wk[j].octave = kps[j].octave;
        wk[j].uright = uright ? uright[j] : -1.0f;
        wk[j].order = (in && !(skip && skip[j])) ? ((unsigned)(px * FRAME_GRID_ROWS + py) << 16) | (unsigned)j : 0xffffffffu;
    }
}

std::mutex g_frame_mu;
std::vector<std::pair<int, char *>> g_frame_pool;     // (capacity, block) of destroyed frames

size_t frame_block_bytes(int cap)
{
    return 256 + ((sizeof(SeqKp) + 32 + 4 + 4) * (size_t)cap + 255) / 256 * 256 + sizeof(int) * (FB_NC + 1);
}

void frame_pointers(orbm_frame *f)
{
    const int cap = f->cap;
    char *p = f->block;
    f->hdr = reinterpret_cast<FrameHdr *>(p); p += 256;
    f->desc = reinterpret_cast<uint4 *>(p); p += (size_t)32 * cap;
    f->kp = reinterpret_cast<SeqKp *>(p); p += sizeof(SeqKp) * (size_t)cap;
    f->angle = reinterpret_cast<float *>(p); p += sizeof(float) * (size_t)cap;
    f->perm = reinterpret_cast<int *>(p);
    f->cell_off = reinterpret_cast<int *>(f->block + frame_block_bytes(cap) - sizeof(int) * (FB_NC + 1));
}

int frame_alloc(orbm_frame *f, int n)
{
    const int cap = std::max(2048, (n + 1023) / 1024 * 1024);
    {
        std::lock_guard<std::mutex> lk(g_frame_mu);
        for (size_t i = 0; i < g_frame_pool.size(); ++i)
            if (g_frame_pool[i].first == cap) {
                f->block = g_frame_pool[i].second;
                g_frame_pool.erase(g_frame_pool.begin() + (long)i);
                break;
            }
    }
    if (!f->block && hipMalloc((void **)&f->block, frame_block_bytes(cap)) != hipSuccess) { f->block = nullptr; return -1; }
    f->cap = cap;
    f->refs = new std::atomic<int>(1);
    frame_pointers(f);
    return 0;
}

void frame_release(orbm_frame *f)
{
    if (f->block && f->refs && f->refs->fetch_sub(1) == 1) {      // the last handle on the block
        delete f->refs;
        {
            std::lock_guard<std::mutex> lk(g_frame_mu);
            if (g_frame_pool.size() < 64) { g_frame_pool.emplace_back(f->cap, f->block); f->block = nullptr; }
        }
        if (f->block) (void)hipFree(f->block);
    }
    delete f;
}

std::atomic<int> g_last_frame_build_waits{0};    // host waits of the last frame-making call (orbm_debug_last_frame_build_waits)

int frame_build_prepare()
{
    static std::atomic<bool> attr_set{false};
    if (!attr_set.load(std::memory_order_acquire)) {
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_frame_build<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS));
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_frame_build<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS));
        attr_set.store(true, std::memory_order_release);
    }
    return ORBX_OK;
}

FrameJob frame_job(const orbm_frame *f, const orbx_keypoint *d_kps, const uint4 *d_desc, const float2 *d_xy, const float *d_ur, const int *d_n,
                   int n_host, int n_bound)
{
    return {d_kps, d_desc, d_xy, d_ur, d_n, n_host, n_bound, f->kp, f->desc, f->angle, f->perm, f->cell_off, f->hdr, nullptr, nullptr};
}

// What the host keeps of a built frame: the header and the permutation as they came back (hdr, perm[n_bound])
int frame_adopt(orbm_frame *f, const void *hdr, const int *perm, int n_bound)
{
    FrameHdr h;
    memcpy(&h, hdr, sizeof(h));
    f->n = h.n; f->ns = h.ns;
    f->min_octave = h.n ? h.min_octave : 0; f->max_octave = h.n ? h.max_octave : -1;
    if (h.n < 0 || h.n > n_bound || h.ns < 0 || h.ns > h.n) ORBX_FAIL(ORBX_ERR_HIP, "frame header out of range");
    f->perm_host.assign(perm, perm + h.n);
    f->inv_host.assign((size_t)h.n, 0);
    for (int sp = 0; sp < h.n; ++sp) {
        const int j = f->perm_host[sp];
        if (j < 0 || j >= h.n) ORBX_FAIL(ORBX_ERR_HIP, "frame permutation out of range");
        f->inv_host[j] = sp;
    }
    return ORBX_OK;
}

// k_frame_build on `st` from device-resident inputs, then the header and the permutation back to the host (one small
// block through the pinned arena of the leased workspace `w`, whose first pin_need bytes must be free for it).
// cam: Frame::UndistortKeyPoints inside the build (null: the coordinates as they are, or d_xy).
int frame_build(orbm_frame *f, Workspace &w, const orbx_keypoint *d_kps, const uint4 *d_desc, const float2 *d_xy, const float *d_ur,
                const int *d_n, int n_host, int n_bound, const orbm_distortion *cam = nullptr)
{
    if (const int rc = frame_build_prepare()) return rc;
    hipStream_t st = w.st;
    hipLaunchKernelGGL(k_frame_build<false>, dim3(1), dim3(FB_T), FB_LDS, st, frame_job(f, d_kps, d_desc, d_xy, d_ur, d_n, n_host, n_bound),
                       (const FrameJob *)nullptr, f->gp, cam ? *cam : orbm_distortion{});
    ORBX_HIP(hipGetLastError());
    // results: hdr (256-byte slot) + perm[n_bound], staged out through the arena's tail
    const size_t bytes = (256 + sizeof(int) * (size_t)n_bound + 15) & ~(size_t)15;
    char *pin = w.pin + w.pin_cap - ((bytes + 255) & ~(size_t)255);
    ORBX_HIP(hipMemcpyAsync(pin, f->hdr, sizeof(FrameHdr), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(pin + 256, f->perm, sizeof(int) * (size_t)n_bound, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    g_last_frame_build_waits.fetch_add(1, std::memory_order_relaxed);      // counted where the stream is waited for
    return frame_adopt(f, pin, reinterpret_cast<const int *>(pin + 256), n_bound);
}

// A frame with room for n keypoints, empty arrays and the grid of the given bounds (null: allocation failed).  nstereo: of a frame
// with right coordinates, how many are >= 0 (-1: they are on the device, not counted)
orbm_frame *frame_new(int n, int has_uright, int nstereo, float min_x, float min_y, float max_x, float max_y)
{
    orbm_frame *f = new orbm_frame();
    f->min_x = min_x; f->min_y = min_y; f->max_x = max_x; f->max_y = max_y; f->has_uright = has_uright; f->nstereo = has_uright ? nstereo : 0;
    f->gp = grid_params(min_x, min_y, max_x, max_y);
    if (frame_alloc(f, n)) { frame_release(f); return nullptr; }
    return f;
}

} // namespace

// A recycled block goes to the next orbm_frame_create as it is: the fill and its wait run under the pool's mutex.
int orbm_detail::frame_pool_fill(uint32_t word)
{
    static hipStream_t st = nullptr;        // the fill's own (guarded by the pool's mutex): never the legacy stream, and no workspace's
    std::lock_guard<std::mutex> lk(g_frame_mu);
    if (g_frame_pool.empty()) return 0;
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = nullptr; return -1; }
    for (const std::pair<int, char *> &b : g_frame_pool)
        if (hipMemsetD32Async((hipDeviceptr_t)b.second, (int)word, frame_block_bytes(b.first) / 4, st) != hipSuccess) return -1;
    return hipStreamSynchronize(st) == hipSuccess ? (int)g_frame_pool.size() : -1;
}

// Keypoints in the grid (and not excluded by `skip`), ordered by (cell, index).
void orbm_detail::sort_frame(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *skip, const float *uright, float min_x,
                             float min_y, float max_x, float max_y, SortedFrame &sf)
{
    std::vector<WinKp> wk;
    sf.gp = grid_params(min_x, min_y, max_x, max_y);
    build_winkp(kps, n, skip, uright, sf.gp, wk);
    // counting sort by grid cell; inside a cell ascending keypoint index (= insertion order, Frame.cc:245-260)
    sf.cell_off.assign(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, 0);
    for (int j = 0; j < n; ++j)
        if (wk[j].order != 0xffffffffu) sf.cell_off[(wk[j].order >> 16) + 1]++;
    for (int c = 0; c < FRAME_GRID_COLS * FRAME_GRID_ROWS; ++c) sf.cell_off[c + 1] += sf.cell_off[c];
    const size_t ns = (size_t)sf.cell_off[FRAME_GRID_COLS * FRAME_GRID_ROWS];
    std::vector<unsigned> order(ns ? ns : 1);
    {
        std::vector<int> fill(sf.cell_off.begin(), sf.cell_off.end() - 1);
        for (int j = 0; j < n; ++j)
            if (wk[j].order != 0xffffffffu) order[fill[wk[j].order >> 16]++] = wk[j].order;
    }
    sf.kp.resize(ns ? ns : 1); sf.perm.resize(ns ? ns : 1); sf.angle.resize(ns ? ns : 1); sf.desc.resize(32 * (ns ? ns : 1));
    for (size_t s = 0; s < ns; ++s) {
        const int j = (int)(order[s] & 0xffffu);
        sf.kp[s] = {wk[j].x, wk[j].y, wk[j].uright, wk[j].octave};
        sf.perm[s] = j;
        sf.angle[s] = kps[j].angle;
        memcpy(&sf.desc[32 * s], desc + 32 * (size_t)j, 32);
    }
    sf.kp.resize(ns); sf.perm.resize(ns); sf.angle.resize(ns); sf.desc.resize(32 * ns);
}

extern "C" {

int orbm_sorted_frame(const orbx_keypoint *kps, int n, const uint8_t *skip, const float *uright, float min_x, float min_y,
                      float max_x, float max_y, int32_t *perm, int32_t *cell_off, int32_t *nsorted)
{
    if (n < 0 || (n && !kps) || !nsorted || !(max_x > min_x) || !(max_y > min_y)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > 65535) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 65,535 keypoints per frame");
    SortedFrame sf;
    std::vector<uint8_t> nodesc((size_t)32 * (n ? n : 1), 0);
    sort_frame(kps, nodesc.data(), n, skip, uright, min_x, min_y, max_x, max_y, sf);
    *nsorted = (int)sf.perm.size();
    if (perm) memcpy(perm, sf.perm.data(), sizeof(int) * sf.perm.size());
    if (cell_off) memcpy(cell_off, sf.cell_off.data(), sizeof(int) * sf.cell_off.size());
    return ORBX_OK;
}

// ------------------------------------------------------------------------------------------------ resident frames

int orbm_frame_create(const orbx_keypoint *kps, const uint8_t *desc, int n, const float *uright, float min_x, float min_y, float max_x,
                      float max_y, orbm_frame **out)
{
    if (!out || n < 0 || (n && (!kps || !desc)) || !(max_x > min_x) || !(max_y > min_y)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > FB_MAXN) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 8,192 keypoints in a resident frame");
    ORBX_NEED_DEVICE();
    g_last_frame_build_waits.store(0, std::memory_order_relaxed);
    int nstereo = 0;
    for (int i = 0; uright && i < n; ++i) nstereo += uright[i] >= 0;
    orbm_frame *f = frame_new(n, uright ? 1 : 0, nstereo, min_x, min_y, max_x, max_y);
    if (!f) ORBX_FAIL(ORBX_ERR_HIP, "frame allocation failed");
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    const size_t m = n ? (size_t)n : 1;
    const size_t o_k = w.carve(sizeof(orbx_keypoint) * m), o_d = w.carve(32 * m), o_u = w.carve(sizeof(float) * m);
    const size_t staged = w.used;
    if (w.reserve(staged, staged + sizeof(int) * m + 1024)) { frame_release(f); ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed"); }
    if (n) {
        memcpy(w.h<char>(o_k), kps, sizeof(orbx_keypoint) * m);
        memcpy(w.h<char>(o_d), desc, 32 * m);
        if (uright) memcpy(w.h<char>(o_u), uright, sizeof(float) * m);
    }
    int rc = orbx::stage_in(w.dev, w.pin, staged, w.st) == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
    if (rc == ORBX_OK)
        rc = frame_build(f, w, w.d<orbx_keypoint>(o_k), w.d<uint4>(o_d), nullptr, uright ? w.d<float>(o_u) : nullptr, nullptr, n, n ? n : 1);
    if (rc != ORBX_OK) { frame_release(f); return rc; }
    *out = f;
    return ORBX_OK;
}

// orbm_frame_from_extractor / orbm_frame_from_extractor_cam: the coordinates from the host (xy_undistorted), through the camera
// inside the build (cam), or as the extractor left them (both null)
static int frame_from_extractor(orbx_extractor *ex, int frame, const float *xy_undistorted, const orbm_distortion *cam, const float *uright,
                                int uright_from_stereo, float min_x, float min_y, float max_x, float max_y, orbm_frame **out)
{
    if (!out || !ex || frame < 0 || frame >= ex->last_batch || !(max_x > min_x) || !(max_y > min_y) || (uright && uright_from_stereo))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (cam && !distortion_ok(*cam)) ORBX_FAIL(ORBX_ERR_ARG, "camera with a non-finite field or a zero focal length");
    if (ex->kcap > FB_MAXN) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 8,192 keypoints in a resident frame");
    if (uright_from_stereo && (!ex->d_uright || !ex->st_valid || frame >= ex->st_batch)) ORBX_FAIL(ORBX_ERR_ARG, "no stereo results");
    ORBX_NEED_DEVICE();
    g_last_frame_build_waits.store(0, std::memory_order_relaxed);
    const int cap = ex->kcap;
    orbm_frame *f = frame_new(cap, (uright || uright_from_stereo) ? 1 : 0, -1, min_x, min_y, max_x, max_y);
    if (!f) ORBX_FAIL(ORBX_ERR_HIP, "frame allocation failed");
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    const size_t o_xy = w.carve(xy_undistorted ? sizeof(float) * 2 * (size_t)cap : 1), o_u = w.carve(uright ? sizeof(float) * (size_t)cap : 1);
    const size_t staged = w.used;
    if (w.reserve(staged, staged + sizeof(int) * (size_t)cap + 1024)) { frame_release(f); ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed"); }
    // the caller's arrays hold n entries, n = the frame's count: known here only after the extraction has finished -- it has, for
    // the caller to hold undistorted coordinates -- so read it back first in that case
    int n_known = -1;
    const int *d_n = ex->d_counts + frame;
    const uint8_t *d_desc = ex->d_desc + (size_t)frame * cap * 32;
    orbx_extractor *producer = orbx_detail::order_after_producer(d_desc, w.st);
    int rc = ORBX_OK;
    if (xy_undistorted || uright) {
        if (hipMemcpyAsync(&n_known, d_n, sizeof(int), hipMemcpyDeviceToHost, w.st) != hipSuccess || hipStreamSynchronize(w.st) != hipSuccess) rc = ORBX_ERR_HIP;
        g_last_frame_build_waits.fetch_add(1, std::memory_order_relaxed);
        if (rc == ORBX_OK && (n_known < 0 || n_known > cap)) rc = ORBX_ERR_HIP;
        if (rc == ORBX_OK) {
            if (xy_undistorted) memcpy(w.h<char>(o_xy), xy_undistorted, sizeof(float) * 2 * (size_t)n_known);
            if (uright) memcpy(w.h<char>(o_u), uright, sizeof(float) * (size_t)n_known);
            if (orbx::stage_in(w.dev, w.pin, staged, w.st) != hipSuccess) rc = ORBX_ERR_HIP;
        }
    }
    if (rc == ORBX_OK)
        rc = frame_build(f, w, ex->d_kps + (size_t)frame * cap, reinterpret_cast<const uint4 *>(d_desc),
                         xy_undistorted ? w.d<float2>(o_xy) : nullptr,
                         uright ? w.d<float>(o_u) : (uright_from_stereo ? ex->d_uright + (size_t)frame * cap : nullptr), d_n, 0, cap, cam);
    (void)producer;      // frame_build has waited for the stream: nothing of this call still reads the extractor's buffers
    if (rc != ORBX_OK) { frame_release(f); if (rc == ORBX_ERR_HIP) ORBX_FAIL(ORBX_ERR_HIP, "building the frame failed"); return rc; }
    *out = f;
    return ORBX_OK;
}

int orbm_frame_from_extractor(orbx_extractor *ex, int frame, const float *xy_undistorted, const float *uright, int uright_from_stereo,
                              float min_x, float min_y, float max_x, float max_y, orbm_frame **out)
{
    return frame_from_extractor(ex, frame, xy_undistorted, nullptr, uright, uright_from_stereo, min_x, min_y, max_x, max_y, out);
}

int orbm_frame_from_extractor_cam(orbx_extractor *ex, int frame, const orbm_distortion *cam, const float *uright, int uright_from_stereo,
                                  float min_x, float min_y, float max_x, float max_y, orbm_frame **out)
{
    return frame_from_extractor(ex, frame, nullptr, cam, uright, uright_from_stereo, min_x, min_y, max_x, max_y, out);
}

int orbm_frames_from_extractor(orbx_extractor *ex, int first, int count, const orbm_distortion *cam, int uright_from_stereo, float min_x,
                               float min_y, float max_x, float max_y, orbm_frame **out)
{
    if (!out || !ex || first < 0 || count < 0 || count > ex->last_batch || first > ex->last_batch - count || !(max_x > min_x) || !(max_y > min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (cam && !distortion_ok(*cam)) ORBX_FAIL(ORBX_ERR_ARG, "camera with a non-finite field or a zero focal length");
    if (ex->kcap > FB_MAXN) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 8,192 keypoints in a resident frame");
    if (uright_from_stereo && (!ex->d_uright || !ex->st_valid || first + count > ex->st_batch)) ORBX_FAIL(ORBX_ERR_ARG, "no stereo results");
    ORBX_NEED_DEVICE();
    g_last_frame_build_waits.store(0, std::memory_order_relaxed);
    if (count == 0) return ORBX_OK;
    const int cap = ex->kcap;
    std::vector<orbm_frame *> fs((size_t)count, nullptr);
    auto fail = [&](int rc, const char *what) {       // all or nothing
        for (orbm_frame *f : fs)
            if (f) frame_release(f);
        ORBX_FAIL(rc, what);
    };
    for (int i = 0; i < count; ++i)
        if (!(fs[i] = frame_new(cap, uright_from_stereo ? 1 : 0, -1, min_x, min_y, max_x, max_y))) return fail(ORBX_ERR_HIP, "frame allocation failed");
    if (frame_build_prepare() != ORBX_OK) return fail(ORBX_ERR_HIP, "building the frames failed");
    // staged: the table of the frames; result block: a 256-byte header slot and perm[cap] per frame
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    const size_t slot = (256 + sizeof(int) * (size_t)cap + 255) & ~(size_t)255;
    const size_t o_tab = w.carve(sizeof(FrameJob) * (size_t)count), staged = w.used, o_res = w.carve(slot * (size_t)count), res_bytes = w.used - o_res;
    const size_t total = w.used;
    if (w.reserve(total, std::max(staged, res_bytes))) return fail(ORBX_ERR_HIP, "workspace allocation failed");
    FrameJob *tab = w.h<FrameJob>(o_tab);
    for (int i = 0; i < count; ++i) {
        const size_t fr = (size_t)(first + i);
        tab[i] = frame_job(fs[i], ex->d_kps + fr * cap, reinterpret_cast<const uint4 *>(ex->d_desc + fr * cap * 32), nullptr,
                           uright_from_stereo ? ex->d_uright + fr * cap : nullptr, ex->d_counts + fr, 0, cap);
        tab[i].res_hdr = reinterpret_cast<FrameHdr *>(w.dev + o_res + slot * i);
        tab[i].res_perm = reinterpret_cast<int *>(w.dev + o_res + slot * i + 256);
    }
    const hipStream_t st = w.st;
    orbx_extractor *producer = orbx_detail::order_after_producer(ex->d_desc + (size_t)first * cap * 32, st);
    bool ok = orbx::stage_in(w.dev, w.pin, staged, st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_frame_build<true>, dim3(count), dim3(FB_T), FB_LDS, st, tab[0], (const FrameJob *)w.d<FrameJob>(o_tab), fs[0]->gp,
                           cam ? *cam : orbm_distortion{});
        ok = hipGetLastError() == hipSuccess && orbx::stage_out(w.pin, w.dev + o_res, res_bytes, st) == hipSuccess;
    }
    ok = hipStreamSynchronize(st) == hipSuccess && ok;     // (waited for in any case: nothing of this call still reads the extractor's buffers)
    g_last_frame_build_waits.store(1, std::memory_order_relaxed);
    (void)producer;
    if (!ok) return fail(ORBX_ERR_HIP, "building the frames failed");
    for (int i = 0; i < count; ++i) {
        const char *r = w.pin + slot * i;
        if (frame_adopt(fs[i], r, reinterpret_cast<const int *>(r + 256), cap) != ORBX_OK) return fail(ORBX_ERR_HIP, "frame header out of range");
    }
    for (int i = 0; i < count; ++i) out[i] = fs[i];
    return ORBX_OK;
}

int orbm_frame_keypoints_un(const orbm_frame *f, float *xy)
{
    if (!f || (f->n && !xy)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (f->n == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    std::vector<SeqKp> kp((size_t)f->n);
    if (const int rc = copy_and_wait({{kp.data(), f->kp, sizeof(SeqKp) * (size_t)f->n}}, hipMemcpyDeviceToHost)) return rc;
    for (int sp = 0; sp < f->n; ++sp) { xy[2 * f->perm_host[sp]] = kp[sp].x; xy[2 * f->perm_host[sp] + 1] = kp[sp].y; }
    return ORBX_OK;
}

int orbm_debug_last_frame_build_waits(void) { return g_last_frame_build_waits.load(std::memory_order_relaxed); }

int orbm_image_bounds(const orbm_distortion *cam, int width, int height, float *bounds)
{
    if (!cam || !bounds || width <= 0 || height <= 0 || !distortion_ok(*cam)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    float x[4], y[4];       // (0, 0), (w, 0), (0, h), (w, h): Frame::ComputeImageBounds (src/Frame.cc:451-479)
    for (int i = 0; i < 4; ++i) undistort_point(*cam, (i & 1) ? (float)width : 0.0f, (i & 2) ? (float)height : 0.0f, &x[i], &y[i]);
    bounds[0] = std::min(x[0], x[2]); bounds[1] = std::min(y[0], y[1]);
    bounds[2] = std::max(x[1], x[3]); bounds[3] = std::max(y[2], y[3]);
    return ORBX_OK;
}

int orbm_undistort_points(const orbm_distortion *cam, const float *xy, int n, float *xy_un)
{
    if (!cam || n < 0 || (n && (!xy || !xy_un)) || !distortion_ok(*cam)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    if (n == 0) return ORBX_OK;
    StagedCall sc;
    const size_t o_in = sc.in(xy, sizeof(float) * 2 * (size_t)n), o_out = sc.out(sizeof(float) * 2 * (size_t)n);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_undistort_points, dim3((n + MT - 1) / MT), dim3(MT), 0, sc.stream(), *cam, (const float2 *)sc.d<float2>(o_in), n,
                       sc.d<float2>(o_out));
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(xy_un, sc.r<float>(o_out), sizeof(float) * 2 * (size_t)n);
    return ORBX_OK;
}

int orbm_frame_destroy(orbm_frame *f)
{
    if (!f) return ORBX_OK;
    frame_release(f);
    return ORBX_OK;
}

int orbm_frame_alias(const orbm_frame *src, float min_x, float min_y, float max_x, float max_y, orbm_frame **out)
{
    if (!src || !out || !(max_x > min_x) || !(max_y > min_y)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    orbm_frame *f = new orbm_frame();
    f->n = src->n; f->ns = src->ns; f->cap = src->cap; f->has_uright = src->has_uright; f->nstereo = src->nstereo;
    f->min_octave = src->min_octave; f->max_octave = src->max_octave;
    f->min_x = min_x; f->min_y = min_y; f->max_x = max_x; f->max_y = max_y;
    f->gp = {min_x, min_y, src->gp.inv_w, src->gp.inv_h};        // KeyFrame: int bounds, the Frame's mfGridElement*Inv (KeyFrame.cc:36,44)
    f->block = src->block; f->refs = src->refs;
    f->refs->fetch_add(1);
    frame_pointers(f);
    f->perm_host = src->perm_host; f->inv_host = src->inv_host;
    *out = f;
    return ORBX_OK;
}

int orbm_frame_size(const orbm_frame *f, int *n, int *nsorted)
{
    if (!f) ORBX_FAIL(ORBX_ERR_ARG, "null frame");
    if (n) *n = f->n;
    if (nsorted) *nsorted = f->ns;
    return ORBX_OK;
}

int orbm_frame_layout(const orbm_frame *f, int32_t *perm, int32_t *cell_off)
{
    if (!f) ORBX_FAIL(ORBX_ERR_ARG, "null frame");
    if (perm) memcpy(perm, f->perm_host.data(), sizeof(int) * (size_t)f->ns);
    if (cell_off) return copy_and_wait({{cell_off, f->cell_off, sizeof(int) * (FB_NC + 1)}}, hipMemcpyDeviceToHost);   // (debug accessor)
    return ORBX_OK;
}

} // extern "C"
