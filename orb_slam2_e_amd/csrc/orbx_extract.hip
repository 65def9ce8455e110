// orbx_extract.hip -- ORB extractor (FAST pyramid + octree + rBRIEF) for gfx950: the handle, the frame plan, the workspace and the calls.
//
// Replaces ORB_SLAM2::ORBextractor (src/ORBextractor.cc, include/ORBextractor.h).
// One batch = B independent frames; every stage is one launch over all frames
// (and, where there is no dependency, all pyramid levels).  Each stage's kernel stands in a unit of its own together with the
// host code that plans for it and launches it (orbx_extract_internal.h):
//
//   orbx_pyramid.hip   k_pyr_level0    copyMakeBorder of the input            (:1135)
//                      k_pyr_resize    resize level l from l-1 + border       (:1128-1131)   x (nlevels-1), or k_pyr_chain: all in one
//   orbx_fast.hip      k_fast_cells    per 30-px cell FAST-9/16 score + NMS + threshold fallback (:789-837)
//   orbx_octree.hip    k_octree        DistributeOctTree as scan-based rounds (:539-763)
//   orbx_blur.hip      k_blur          GaussianBlur 7x7 sigma 2               (:1093-1094)
//   orbx_describe.hip  k_describe      IC_Angle + steered BRIEF + output      (:77-147, :845-860, :1103-1111)
//
// HBM layout: per frame one pyramid block; level l is a padded image of
// (h_l + 38) rows x stride_l bytes, inner pixel (x, y) at off_l + (y+19)*stride_l + 32 + x
// (19-px REFLECT_101 border as in mvImagePyramid; 32-byte left pad keeps inner
// rows dword/16-B aligned).  All integer work is bit-exact by construction; the
// float steps (fastAtan2, rBRIEF rotation) use fixed IEEE op sequences (orbx_math.h,
// built with -ffp-contract=off).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "orbx_extract_internal.h"

using namespace orbx_detail;

namespace {

void drop_graph(orbx_extractor *ex)
{
    if (ex->g_exec) (void)hipGraphExecDestroy(ex->g_exec);
    if (ex->g_graph) (void)hipGraphDestroy(ex->g_graph);
    ex->g_exec = nullptr; ex->g_graph = nullptr; ex->g_w = ex->g_h = ex->g_stride = 0;
}

void free_workspace(orbx_extractor *ex)
{
    drop_graph(ex);
    const auto drop = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    drop(ex->d_chain); drop(ex->d_chain_tabs); drop(ex->d_chain_span); drop(ex->d_pyr); drop(ex->d_blur); drop(ex->d_lv); drop(ex->d_cells); drop(ex->d_tiles);
    drop(ex->d_blur_frag); drop(ex->d_xt); drop(ex->d_yt); drop(ex->d_cell_count); drop(ex->d_level_count); drop(ex->d_level_ncand); drop(ex->d_counts);
    drop(ex->d_cands); drop(ex->d_kpos); drop(ex->d_sel); drop(ex->d_knode); drop(ex->d_kq); drop(ex->d_desc); drop(ex->d_kps);
    ex->width = ex->height = ex->batch = 0;
}

// A *_dev consumer on another stream (the stereo matcher, a *_dev matcher call) may still read the last batch's results
// (order_after_producer): the next batch on `st` waits for it.
int wait_pending_reader(orbx_extractor *ex, hipStream_t st)
{
    if (ex->reader_pending) {
        if (ex->reader_stream != st) ORBX_HIP(hipStreamWaitEvent(st, ex->reader_ev, 0));
        ex->reader_pending = false;
    }
    return ORBX_OK;
}

// The one-frame call's pinned result block: {count, 12 bytes | kps[kcap], rounded up to 16 bytes | desc[kcap][32]}; the descriptors' offset.
size_t result_desc_off(const orbx_extractor *ex) { return 16 + ((sizeof(orbx_keypoint) * (size_t)ex->kcap + 15) & ~(size_t)15); }

// One frame's results into the caller's pinned block: {count, 0, 0, 0}, the keypoint records, the descriptors -- written by the
// queue that produced them (posted writes over PCIe), 16 bytes per lane.
__global__ __launch_bounds__(256) void k_result_out(const int *__restrict__ counts, const uint4 *__restrict__ kps, const uint4 *__restrict__ desc,
                                                    int kps16, int desc16, uint4 *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) out[0] = make_uint4((unsigned)counts[0], 0u, 0u, 0u);
    if (i < kps16) out[1 + i] = kps[i];
    else if (i < kps16 + desc16) out[1 + i] = desc[i - kps16];
}

std::mutex g_reg_mu;
std::vector<orbx_extractor *> g_reg;   // live handles (orbx_create .. orbx_destroy)

} // namespace

namespace orbx_detail {

orbx_extractor *order_after_producer(const void *ptr, hipStream_t st)
{
    const uint8_t *q = (const uint8_t *)ptr;
    orbx_extractor *hit = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        for (orbx_extractor *ex : g_reg) {
            if (!ex->d_desc || !ex->batch) continue;
            const size_t B = (size_t)ex->batch, cap = (size_t)ex->kcap;
            const uint8_t *d = ex->d_desc, *k = (const uint8_t *)ex->d_kps, *c = (const uint8_t *)ex->d_counts;
            if ((q >= d && q < d + B * cap * 32) || (q >= k && q < k + B * cap * sizeof(orbx_keypoint)) || (q >= c && q < c + B * sizeof(int))) {
                hit = ex;
                break;
            }
        }
    }
    if (!hit || !hit->last_batch || hit->last_stream == st) return nullptr;
    if (!hit->order_ev && hipEventCreateWithFlags(&hit->order_ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    // everything queued on the producer's stream so far -- its last batch was queued by an earlier call -- precedes `st`'s next work
    if (hipEventRecord(hit->order_ev, hit->last_stream) != hipSuccess || hipStreamWaitEvent(st, hit->order_ev, 0) != hipSuccess) return nullptr;
    return hit;
}

void reader_done(orbx_extractor *ex, hipStream_t st)
{
    if (!ex) return;
    if (!ex->reader_ev && hipEventCreateWithFlags(&ex->reader_ev, hipEventDisableTiming) != hipSuccess) return;
    if (hipEventRecord(ex->reader_ev, st) != hipSuccess) return;
    ex->reader_stream = st;
    ex->reader_pending = true;
}

#ifdef ORBX_PHASE_TIMING
int phase_quarter(void *rec, unsigned long long *out, int reset)   // one unit's 65536 x 16 records (ORBX_PHASE_UNIT)
{
    const size_t bytes = sizeof(unsigned long long) * 65536 * 16;
    hipStream_t st = nullptr;   // (a stream of its own: nothing in this library touches the legacy stream)
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return -1;
    bool ok = !out || hipMemcpyAsync(out, rec, bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && (!reset || hipMemsetAsync(rec, 0, bytes, st) == hipSuccess) && hipStreamSynchronize(st) == hipSuccess;
    (void)hipStreamDestroy(st);
    return ok ? 0 : -1;
}
#endif

} // namespace orbx_detail

extern "C" {

const char *orbx_last_error(void) { return orbx::last_error().c_str(); }
int orbx_abi_version(void) { return 136; } // 136: + orbm_pose_optimization, orbm_frame_pose_optimization, orbm_pose_optimization_batch, orbm_pose_camera, orbm_pose_stats (additions only); 135: + orbm_profile_read_bow (addition only); 134: + fem_cg_one_launch_stats (addition only); 133: + fem_plan_single_cg (addition only); 132: + fem_cg_preconditioner, fem_cg_coarse_matrix (additions only); 131: + orbm_frame_search_by_bow, orbm_frame_search_for_triangulation; ORBM_ALLPAIRS_MFMA now names the second matrix-core kernel (additions only); 130: + orbm_frame_*, the whole-function searches, orbx_params.trig_variant (a struct field: rebuild callers); 120: + fem_plan, fem_plan_selfcheck, orbm_sorted_frame, orbx_stereo_download_batch, orbm_debug_* (additions only); 110: + orbm_project_points, fem_create_batch, fem_batch_offsets

int orbx_create(const orbx_params *prm, orbx_extractor **out)
{
    if (!prm || !out) ORBX_FAIL(ORBX_ERR_ARG, "null argument");
    if (prm->nlevels < 1 || prm->nlevels > MAXL || prm->nfeatures < 0 || !(prm->scale_factor > 1.0f) || prm->blur_variant < 0 ||
        prm->blur_variant > 1 || prm->trig_variant < 0 || prm->trig_variant > 1)
        ORBX_FAIL(ORBX_ERR_ARG, "bad extractor parameters");
    orbx_extractor *ex = new orbx_extractor();
    ex->prm = *prm;
    const int nl = ex->nlevels = prm->nlevels;
    // ORBextractor::ORBextractor, ORBextractor.cc:415-446
    ex->scale[0] = 1.0f; ex->sigma2[0] = 1.0f;
    for (int i = 1; i < nl; i++) {
        ex->scale[i] = ex->scale[i - 1] * prm->scale_factor;
        ex->sigma2[i] = ex->scale[i] * ex->scale[i];
    }
    for (int i = 0; i < nl; i++) {
        ex->inv_scale[i] = 1.0f / ex->scale[i];
        ex->inv_sigma2[i] = 1.0f / ex->sigma2[i];
    }
    const float factor = 1.0f / prm->scale_factor;
    float nDesired = prm->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        ex->nfeat[l] = cv_round_f(nDesired);
        sum += ex->nfeat[l];
        nDesired *= factor;
    }
    ex->nfeat[nl - 1] = prm->nfeatures - sum > 0 ? prm->nfeatures - sum : 0;
    for (int l = 0; l < nl; l++)
        if (ex->nfeat[l] > OCT_MAXN) {
            delete ex;
            ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "per-level feature quota above 2047 is not supported");
        }
    if (prm->blur_variant == 1) { ex->taps[0] = 18; ex->taps[1] = 34; ex->taps[2] = 49; ex->taps[3] = 55; }
    else { ex->taps[0] = 18; ex->taps[1] = 34; ex->taps[2] = 48; ex->taps[3] = 56; }
    // DistributeOctTree returns at most N + 3 keypoints for a quota N >= 1 (the last split may overshoot by three) -- and up to
    // four per INITIAL node whatever N is: every initial node is split before the first "enough nodes" test
    // (ORBextractor.cc:575-669).  The number of initial nodes is round(width / height) of the level (:543), known once the
    // frame size is (orbx_reserve raises the capacity if 4 nIni exceeds N + 3 on some level: tiny quotas on wide frames)
    ex->kcap_params = prm->nfeatures + 3 * nl;
    for (int l = 0; l < nl; l++) ex->kcap_params += ex->nfeat[l] == 0 ? 1 : 0;
    ex->kcap = ex->kcap_params;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_reg.push_back(ex);
    }
    *out = ex;
    return ORBX_OK;
}

int orbx_destroy(orbx_extractor *ex)
{
    if (!ex) return ORBX_OK;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_reg.erase(std::remove(g_reg.begin(), g_reg.end(), ex), g_reg.end());
    }
    if (ex->reader_pending) (void)hipEventSynchronize(ex->reader_ev);   // a consumer on another stream may still read the results
    if (ex->order_ev) (void)hipEventDestroy(ex->order_ev);
    if (ex->reader_ev) (void)hipEventDestroy(ex->reader_ev);
    free_workspace(ex);
    if (ex->d_in) (void)hipFree(ex->d_in);
    void *stp[] = {ex->d_st_key, ex->d_st_rk, ex->d_st_rowoff, ex->d_st_items, ex->d_uright, ex->d_depth, ex->d_st_scale, ex->d_st_sad, ex->d_st_nvalid};
    for (void *q : stp)
        if (q) (void)hipFree(q);
    if (ex->h_pin) (void)hipHostFree(ex->h_pin);
    if (ex->h_st_pin) (void)hipHostFree(ex->h_st_pin);
    if (ex->stream) (void)hipStreamDestroy(ex->stream);
    delete ex;
    return ORBX_OK;
}

int orbx_get_levels(const orbx_extractor *ex) { return ex ? ex->nlevels : ORBX_ERR_ARG; }
#define ORBX_GETTER(name, field, type)                                   \
    int name(const orbx_extractor *ex, type *out)                        \
    {                                                                    \
        if (!ex || !out) ORBX_FAIL(ORBX_ERR_ARG, "null argument");       \
        for (int i = 0; i < ex->nlevels; i++) out[i] = ex->field[i];     \
        return ORBX_OK;                                                  \
    }
ORBX_GETTER(orbx_get_scale_factors, scale, float)
ORBX_GETTER(orbx_get_inv_scale_factors, inv_scale, float)
ORBX_GETTER(orbx_get_level_sigma2, sigma2, float)
ORBX_GETTER(orbx_get_inv_level_sigma2, inv_sigma2, float)
ORBX_GETTER(orbx_get_features_per_level, nfeat, int32_t)
int orbx_keypoint_capacity(const orbx_extractor *ex) { return ex ? ex->kcap : ORBX_ERR_ARG; }

int orbx_level_size(const orbx_extractor *ex, int level, int *w, int *h)
{
    if (!ex || level < 0 || level >= ex->nlevels || !ex->width) ORBX_FAIL(ORBX_ERR_ARG, "bad level / nothing reserved");
    if (w) *w = ex->lv[level].w;
    if (h) *h = ex->lv[level].h;
    return ORBX_OK;
}


// Everything orbx_reserve decides about a frame size on the HOST: level geometry, the FAST cell grid, the octree's initial nodes,
// slot / node / result capacities, and -- through the stage units' planners -- resize coefficient tables, blur tiles, LDS budgets.
// No device call (orbx_plan runs it without a GPU: the CPU tests and the host sanitizer pass check its capacities against the
// oracle's literal algorithm).  The per-level loop with its running offsets is here and nowhere else.
static int plan_frame(orbx_extractor *ex, int width, int height, std::vector<int2> &xt, std::vector<int4> &yt)
{
    const int nl = ex->nlevels;
    xt.clear(); yt.clear();
    ex->cells.clear(); ex->tiles.clear();
    size_t off = 0, cand_off = 0, key_off = 0;
    int sel_off = 0, maxcw = 0, maxch = 0, kneed = 0;
    size_t boff_run = 0;
    ex->maxcells = 0;
    for (int l = 0; l < nl; l++) {
        LevelInfo &lv = ex->lv[l];
        memset(&lv, 0, sizeof(lv));
        // ComputePyramid, ORBextractor.cc:1119-1121
        lv.w = cv_round_f((float)width * ex->inv_scale[l]);
        lv.h = cv_round_f((float)height * ex->inv_scale[l]);
        if (lv.w > 4000 || lv.h > 4000) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "image larger than 4000 px");
        lv.stride = (PADX + lv.w + EDGE + 63) & ~63;
        lv.off = (int)off;
        off += (size_t)lv.stride * (lv.h + 2 * EDGE);
        off = (off + 255) & ~(size_t)255;
        // the same level in the blurred buffer's strip layout: stride / 16 strips of ((rows + 7) & ~7) x 16 bytes
        ex->bcol[l] = ((lv.h + 2 * EDGE + 7) & ~7) * 16;
        ex->boff[l] = (int)boff_run;
        boff_run += (size_t)(lv.stride / 16) * ex->bcol[l];
        lv.scale = ex->scale[l];
        lv.patch = (int)(31 * ex->scale[l]); // :845
        lv.N = ex->nfeat[l];
        // ComputeKeyPointsOctTree grid, :773-787
        const int maxBorderX = lv.w - EDGE + 3, maxBorderY = lv.h - EDGE + 3;
        const float fw = (float)(maxBorderX - MIN_BORDER), fh = (float)(maxBorderY - MIN_BORDER);
        const int nCols = (int)(fw / 30.f), nRows = (int)(fh / 30.f);
        if (nCols < 1 || nRows < 1) ORBX_FAIL(ORBX_ERR_ARG, "image too small for the 30-px FAST cell grid at some level");
        const int wCell = (int)ceilf(fw / nCols), hCell = (int)ceilf(fh / nRows);
        lv.W = maxBorderX - MIN_BORDER;
        lv.H = maxBorderY - MIN_BORDER;
        lv.nIni = (int)roundf((float)lv.W / lv.H); // :543
        if (lv.nIni < 1) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "aspect ratio below 0.5 (reference divides by zero)");
        lv.hX = (float)lv.W / lv.nIni;
        lv.cell_base = (int)ex->cells.size();
        lv.key_base = (int)key_off;
        for (int i = 0; i < nRows; i++) { // :789-806
            const float iniY = (float)(MIN_BORDER + i * hCell);
            float maxY = iniY + hCell + 6;
            if (iniY >= maxBorderY - 3) continue;
            if (maxY > maxBorderY) maxY = (float)maxBorderY;
            for (int j = 0; j < nCols; j++) {
                const float iniX = (float)(MIN_BORDER + j * wCell);
                float maxX = iniX + wCell + 6;
                if (iniX >= maxBorderX - 6) continue;
                if (maxX > maxBorderX) maxX = (float)maxBorderX;
                CellInfo c;
                memset(&c, 0, sizeof(c));
                c.level = (short)l;
                c.x0 = (short)(int)iniX; c.y0 = (short)(int)iniY;
                c.cw = (short)((int)maxX - (int)iniX); c.ch = (short)((int)maxY - (int)iniY);
                c.dx = (short)(j * wCell); c.dy = (short)(i * hCell);
                const int zw = c.cw - 6, zh = c.ch - 6;
                c.cap = (zw > 0 && zh > 0) ? ((zw + 1) / 2) * ((zh + 1) / 2) : 0; // 3x3 strict NMS bound
                if (zw > 63 || zh > 63) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "FAST cell larger than 63 px");
                c.ngx = (short)(zw > 0 ? (zw + 3) >> 2 : 1);
                c.qstep = (short)(64 / c.ngx); c.rstep = (short)(64 - c.qstep * c.ngx);
                c.inv_ngx = (65536 + c.ngx - 1) / c.ngx;
                c.stride = lv.stride;
                c.img_off = lv.off + (c.y0 + EDGE) * lv.stride + PADX + (c.x0 - 5);
                c.cand_off = (int)cand_off;
                cand_off += c.cap;
                key_off += c.cap;
                if (c.cw > maxcw) maxcw = c.cw;
                if (c.ch > maxch) maxch = c.ch;
                ex->cells.push_back(c);
            }
        }
        lv.ncells = (int)ex->cells.size() - lv.cell_base;
        if (lv.ncells > ex->maxcells) ex->maxcells = lv.ncells;
        lv.sel_base = sel_off;
        sel_off += level_slots(lv);
        kneed += std::max(lv.N + 3, 4 * lv.nIni);
        int rc = plan_blur(ex, l);
        if (rc == ORBX_OK) rc = plan_pyramid(ex, l, xt, yt);
        if (rc != ORBX_OK) return rc;
    }
    ex->frame_bytes = off;
    ex->blur_frame_bytes = (boff_run + 255) & ~(size_t)255;
    ex->cands_per_frame = cand_off;
    ex->keys_per_frame = key_off;
    ex->cells_per_frame = (int)ex->cells.size();
    ex->sel_per_frame = sel_off;
    ex->kcap = std::max(ex->kcap_params, kneed);
    int rc = plan_fast(ex, maxcw, maxch);
    if (rc == ORBX_OK) rc = plan_octree(ex);
    if (rc == ORBX_OK) rc = plan_chain(ex, xt, yt);
    return rc;
}

int orbx_reserve(orbx_extractor *ex, int width, int height, int batch)
{
    if (!ex || width <= 0 || height <= 0 || batch <= 0) ORBX_FAIL(ORBX_ERR_ARG, "bad reserve arguments");
    ORBX_NEED_DEVICE();
    if (ex->width == width && ex->height == height && ex->batch >= batch) return ORBX_OK;
    if (!ex->stream) ORBX_HIP(hipStreamCreateWithFlags(&ex->stream, hipStreamNonBlocking));
    ORBX_HIP(hipStreamSynchronize(ex->stream));
    free_workspace(ex);
    ex->st_valid = false;   // stereo results were laid out with the old capacity and belong to the old counts
    std::vector<int2> xt;
    std::vector<int4> yt;
    if (const int rc = plan_frame(ex, width, height, xt, yt); rc != ORBX_OK) return rc;

    // every fill and upload below runs on the handle's own stream and is waited for there: a blocking copy on the legacy stream
    // would wait for every other thread's work and fails outright while any thread captures a graph (hipErrorStreamCaptureImplicit)
    const size_t B = (size_t)batch;
    ORBX_HIP(hipMalloc(&ex->d_pyr, ex->frame_bytes * B));
    ORBX_HIP(hipMemsetAsync(ex->d_pyr, 0, ex->frame_bytes * B, ex->stream)); // the row padding outside the 19-px border is never written by k_pyr_resize
    ORBX_HIP(hipMalloc(&ex->d_blur, ex->blur_frame_bytes * B));
    ORBX_HIP(hipMemsetAsync(ex->d_blur, 0, ex->blur_frame_bytes * B, ex->stream));
    ORBX_HIP(hipMalloc(&ex->d_lv, sizeof(LevelInfo) * MAXL));
    {
        int dev = 0, ncu = 0;
        ORBX_HIP(hipGetDevice(&dev));
        ORBX_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
        if (ncu > 0) ex->resident_waves = 32 * ncu;
    }
    ORBX_HIP(hipMalloc(&ex->d_cells, sizeof(CellInfo) * ex->cells.size()));
    ORBX_HIP(hipMalloc(&ex->d_tiles, sizeof(BlurTile) * ex->tiles.size()));
    if (ex->chain_tiles) {
        ORBX_HIP(hipMalloc(&ex->d_chain, sizeof(ChainTile) * ex->chain.size()));
        ORBX_HIP(hipMemcpyAsync(ex->d_chain, ex->chain.data(), sizeof(ChainTile) * ex->chain.size(), hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMalloc(&ex->d_chain_tabs, sizeof(uint4) * ex->chain_tabs.size()));
        ORBX_HIP(hipMemcpyAsync(ex->d_chain_tabs, ex->chain_tabs.data(), sizeof(uint4) * ex->chain_tabs.size(), hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMalloc(&ex->d_chain_span, sizeof(int2) * ex->chain_span.size()));
        ORBX_HIP(hipMemcpyAsync(ex->d_chain_span, ex->chain_span.data(), sizeof(int2) * ex->chain_span.size(), hipMemcpyHostToDevice, ex->stream));
    }
    if (const int rc = prepare_chain(ex); rc != ORBX_OK) return rc;

    ORBX_HIP(hipMalloc(&ex->d_xt, sizeof(int2) * (xt.size() + 1)));
    ORBX_HIP(hipMalloc(&ex->d_yt, sizeof(int4) * (yt.size() + 1)));
    ORBX_HIP(hipMalloc(&ex->d_cell_count, sizeof(int) * ex->cells_per_frame * B));
    ORBX_HIP(hipMalloc(&ex->d_level_count, sizeof(int) * MAXL * B));
    ORBX_HIP(hipMalloc(&ex->d_level_ncand, sizeof(int) * MAXL * B));
    ORBX_HIP(hipMalloc(&ex->d_counts, sizeof(int) * B));
    ORBX_HIP(hipMalloc(&ex->d_cands, sizeof(uint32_t) * ex->cands_per_frame * B));
    ORBX_HIP(hipMalloc(&ex->d_kpos, sizeof(uint32_t) * ex->keys_per_frame * B));
    ORBX_HIP(hipMalloc(&ex->d_knode, sizeof(unsigned short) * ex->keys_per_frame * B));
    ORBX_HIP(hipMalloc(&ex->d_kq, ex->keys_per_frame * B));
    ORBX_HIP(hipMalloc(&ex->d_sel, sizeof(uint32_t) * ((size_t)ex->sel_per_frame * B + DESC_KPB)));   // k_describe reads whole chunks of 16 slots
    ORBX_HIP(hipMalloc(&ex->d_kps, sizeof(orbx_keypoint) * ex->kcap * B + 16));   // (+ 16: k_result_out reads whole 16-byte pieces)
    ORBX_HIP(hipMalloc(&ex->d_desc, (size_t)32 * ex->kcap * B));
    ORBX_HIP(hipMemcpyAsync(ex->d_lv, ex->lv, sizeof(LevelInfo) * MAXL, hipMemcpyHostToDevice, ex->stream));
    ORBX_HIP(hipMemcpyAsync(ex->d_cells, ex->cells.data(), sizeof(CellInfo) * ex->cells.size(), hipMemcpyHostToDevice, ex->stream));
    ORBX_HIP(hipMemcpyAsync(ex->d_tiles, ex->tiles.data(), sizeof(BlurTile) * ex->tiles.size(), hipMemcpyHostToDevice, ex->stream));
    if (const int rc = prepare_blur(ex); rc != ORBX_OK) return rc;
    if (!xt.empty()) ORBX_HIP(hipMemcpyAsync(ex->d_xt, xt.data(), sizeof(int2) * xt.size(), hipMemcpyHostToDevice, ex->stream));
    if (!yt.empty()) ORBX_HIP(hipMemcpyAsync(ex->d_yt, yt.data(), sizeof(int4) * yt.size(), hipMemcpyHostToDevice, ex->stream));
    ORBX_HIP(hipStreamSynchronize(ex->stream));
    if (const int rc = prepare_octree(ex); rc != ORBX_OK) return rc;
    ex->width = width; ex->height = height; ex->batch = batch;
    return ORBX_OK;
}

int orbx_plan(const orbx_params *prm, int width, int height, orbx_plan_info *info)
{
    if (!prm || !info || width <= 0 || height <= 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    orbx_extractor *ex = nullptr;
    int rc = orbx_create(prm, &ex);
    if (rc != ORBX_OK) return rc;
    std::vector<int2> xt;
    std::vector<int4> yt;
    rc = plan_frame(ex, width, height, xt, yt);
    if (rc == ORBX_OK) {
        memset(info, 0, sizeof(*info));
        info->nlevels = ex->nlevels; info->keypoint_capacity = ex->kcap; info->octree_nodes = ex->NC; info->cells_per_frame = ex->cells_per_frame;
        info->sel_per_frame = ex->sel_per_frame; info->fast_tile_stride = ex->TS; info->fast_lds = ex->fast_lds; info->octree_lds = ex->oct_lds;
        info->octree_kshift = ex->oct_kshift; info->frame_bytes = (int64_t)ex->frame_bytes; info->cands_per_frame = (int64_t)ex->cands_per_frame;
        for (int l = 0; l < ex->nlevels; l++) {
            const LevelInfo &lv = ex->lv[l];
            info->level_w[l] = lv.w; info->level_h[l] = lv.h; info->level_quota[l] = lv.N; info->level_nini[l] = lv.nIni;
            info->level_slots[l] = level_slots(lv); info->level_cells[l] = lv.ncells;
        }
    }
    orbx_destroy(ex);
    return rc;
}

int orbx_debug_fast_pieces(const orbx_params *prm, int width, int height, int32_t *out, int cap, int *n)
{
    if (!prm || !out || !n || width <= 0 || height <= 0 || cap < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    orbx_extractor *ex = nullptr;
    int rc = orbx_create(prm, &ex);
    if (rc != ORBX_OK) return rc;
    std::vector<int2> xt;
    std::vector<int4> yt;
    rc = plan_frame(ex, width, height, xt, yt);
    if (rc == ORBX_OK) rc = debug_fast_pieces(ex, out, cap, n);
    orbx_destroy(ex);
    return rc;
}

int orbx_extract_batch(orbx_extractor *ex, const uint8_t *images, int is_device, int width, int height, int stride,
                       size_t frame_stride, int batch, void *stream_)
{
    if (!ex || !images || width <= 0 || height <= 0 || batch <= 0 || stride < width)
        ORBX_FAIL(ORBX_ERR_ARG, "bad extract arguments");
    ORBX_NEED_DEVICE();
    int rc = orbx_reserve(ex, width, height, batch);
    if (rc != ORBX_OK) return rc;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : ex->stream;
    rc = wait_pending_reader(ex, st);
    if (rc != ORBX_OK) return rc;
    const uint8_t *d_img = images;
    if (!is_device) {
        const size_t need = frame_stride * (size_t)(batch - 1) + (size_t)stride * height;
        if (need > ex->in_bytes) {
            if (ex->d_in) ORBX_HIP(hipFree(ex->d_in));
            ex->d_in = nullptr;
            ORBX_HIP(hipMalloc(&ex->d_in, need));
            ex->in_bytes = need;
        }
        // (what is copied ends with the last pixel of the last row: a cv::Mat with a row pitch -- a region of interest at the bottom of its
        // parent -- owns nothing behind it)
        ORBX_HIP(hipMemcpyAsync(ex->d_in, images, need - (size_t)(stride - width), hipMemcpyHostToDevice, st));
        d_img = ex->d_in;
    }
    launch_level0(ex, d_img, stride, frame_stride, batch, st);
    launch_pyramid(ex, batch, st);
    launch_fast(ex, batch, st);
    launch_octree(ex, batch, st);
    launch_blur(ex, batch, st);
    launch_describe(ex, batch, st);
    ORBX_HIP(hipGetLastError());
    ex->last_batch = batch;
    ex->last_stream = st;
    return ORBX_OK;
}

int orbx_profile_enable(orbx_extractor *ex, int on)
{
    if (!ex) ORBX_FAIL(ORBX_ERR_ARG, "null argument");
    static const char *names[6] = {"k_pyr_level0", "k_pyr_resize", "k_fast_cells", "k_octree", "k_blur", "k_describe"};
    for (int i = 0; i < 6; ++i) ex->prof.names[i] = names[i];
    ex->prof.reset();
    ex->prof.mask = on < 0 ? 0xffffu : (unsigned)on;
    return ORBX_OK;
}

#ifdef ORBX_PHASE_TIMING
int orbx_debug_phases(unsigned long long *out, int reset)   // out: 4 x 65536 x 16 records (FAST, describe, pyramid, octree)
{
    const size_t q = (size_t)65536 * 16;
    const bool ok = phases_fast(out, reset) == 0 && phases_describe(out ? out + q : nullptr, reset) == 0 &&
                    phases_pyramid(out ? out + 2 * q : nullptr, reset) == 0 && phases_octree(out ? out + 3 * q : nullptr, reset) == 0;
    return ok ? 0 : -1;
}
#endif

int orbx_profile_read(orbx_extractor *ex, int max_kinds, const char **names, double *total_ms, int64_t *launches, int *nkinds)
{
    if (!ex || !nkinds) ORBX_FAIL(ORBX_ERR_ARG, "null argument");
    ex->prof.flush();
    int n = 0;
    for (int i = 0; i < orbx::KernelProfiler::MAXK && n < max_kinds; ++i) {
        if (!ex->prof.names[i]) continue;
        if (names) names[n] = ex->prof.names[i];
        if (total_ms) total_ms[n] = ex->prof.ms[i];
        if (launches) launches[n] = ex->prof.launches[i];
        ++n;
    }
    *nkinds = n;
    return ORBX_OK;
}

int orbx_download(orbx_extractor *ex, int frame, orbx_keypoint *kps, uint8_t *desc, int cap, int *n)
{
    if (!ex || frame < 0 || frame >= ex->last_batch || !n) ORBX_FAIL(ORBX_ERR_ARG, "bad download arguments");
    // copies queued behind the batch on ITS stream and one wait for that stream: the other SLAM threads' streams
    // (LocalMapping, LoopClosing) are not stalled, as a device-wide synchronisation would
    hipStream_t st = ex->last_stream;
    int cnt = 0;
    ORBX_HIP(hipMemcpyAsync(&cnt, ex->d_counts + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    *n = cnt;
    if (cnt > cap) ORBX_FAIL(ORBX_ERR_CAPACITY, "keypoint buffer too small");
    if (cnt > 0) {
        if (kps) ORBX_HIP(hipMemcpyAsync(kps, ex->d_kps + (size_t)frame * ex->kcap, sizeof(orbx_keypoint) * cnt, hipMemcpyDeviceToHost, st));
        if (desc) ORBX_HIP(hipMemcpyAsync(desc, ex->d_desc + (size_t)frame * ex->kcap * 32, (size_t)32 * cnt, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
    }
    return ORBX_OK;
}

int orbx_download_batch(orbx_extractor *ex, orbx_keypoint *kps, uint8_t *desc, int32_t *counts)
{
    if (!ex || ex->last_batch <= 0 || !ex->d_kps) ORBX_FAIL(ORBX_ERR_ARG, "no results");
    hipStream_t st = ex->last_stream;
    const size_t B = (size_t)ex->last_batch;
    if (counts) ORBX_HIP(hipMemcpyAsync(counts, ex->d_counts, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    if (kps) ORBX_HIP(hipMemcpyAsync(kps, ex->d_kps, sizeof(orbx_keypoint) * ex->kcap * B, hipMemcpyDeviceToHost, st));
    if (desc) ORBX_HIP(hipMemcpyAsync(desc, ex->d_desc, (size_t)32 * ex->kcap * B, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return ORBX_OK;
}

// One host image through the extractor, in two halves: everything up to the last launch (extract_enqueue), and the wait + the copy
// out of the pinned block (extract_finish).  orbx_extract is one after the other; orbx_extract_pair enqueues the left and the right
// image of a stereo frame on their two handles' streams before it waits for either.
static int extract_enqueue(orbx_extractor *ex, const uint8_t *image, int width, int height, int stride, bool as_graph = false)
{
    // ORBextractor::operator() on one host image is latency-bound: stage the image and the results through pinned
    // buffers so that the call is one H2D, the kernel chain, one D2H and a single stream synchronisation
    if (stride < width) ORBX_FAIL(ORBX_ERR_ARG, "row pitch smaller than the width");
    const size_t in_bytes = (size_t)stride * height, in_room = (in_bytes + 255) & ~(size_t)255;   // 16-byte pieces on both sides
    int rc = orbx_reserve(ex, width, height, 1);
    if (rc != ORBX_OK) return rc;
    const size_t desc_off = result_desc_off(ex), out_bytes = desc_off + (size_t)32 * ex->kcap;
    if (in_room + out_bytes > ex->pin_bytes) {
        drop_graph(ex);
        if (ex->h_pin) (void)hipHostFree(ex->h_pin);
        ex->h_pin = nullptr; ex->pin_bytes = 0;
        ORBX_HIP(hipHostMalloc((void **)&ex->h_pin, in_room + out_bytes, hipHostMallocDefault));
        ex->pin_bytes = in_room + out_bytes;
    }
    hipStream_t st = ex->stream;
    rc = wait_pending_reader(ex, st);
    if (rc != ORBX_OK) return rc;
    // An image that already lies in pinned (hipHostMalloc'ed or hipHostRegister'ed) memory -- a capture buffer the caller allocated that way --
    // is read where it is: no staging copy (10 us of a 111-us call for 640 x 480).  Not for the pair call's captured graph, whose kernel
    // arguments are fixed.
    const uint8_t *src = ex->h_pin;
    if (!as_graph) {
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, image) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer) src = static_cast<const uint8_t *>(pa.devicePointer);
        else (void)hipGetLastError();
    }
    if (src == ex->h_pin) memcpy(ex->h_pin, image, in_bytes - (size_t)(stride - width));   // (ends with the last row's last pixel: a region of interest owns nothing behind it)
    ex->pin_result_off = in_room;
    // image in and results out by the compute queue itself (the kernels read / write the pinned block): no hand-over to the copy engine
    // in front of and behind the kernels of a frame
    auto enqueue = [&]() -> int {
        // (level 0 reads the pinned image itself -- it is mapped into the device's address space --: 16 us instead of a staging copy + 7, and
        // one launch less; 0.149 -> 0.146 ms per call)
        // (the results: k_describe stores every record into the pinned block as well -- no copy kernel behind it)
        ex->mirror = reinterpret_cast<uint32_t *>(ex->h_pin + in_room); ex->mirror_desc = (int)(desc_off / 4);
        const int rc2 = orbx_extract_batch(ex, src, 1, width, height, stride, in_bytes, 1, st);
        ex->mirror = nullptr;
        if (rc2 != ORBX_OK) return rc2;
        return ORBX_OK;
    };
    // As a graph (orbx_extract_pair): the launches of a frame (fourteen when this was written, seven now) cost the host time to enqueue, which is what the SECOND
    // image of a stereo frame waits for; one graph launch per image lets the two chains run side by side on the device.  Captured
    // on the second call of a frame size (the first has done every one-time set-up), only while nothing in the chain depends on
    // the call (no per-kernel profiling events; a pending reader of the last results is waited for in front of the chain); any
    // failure falls back to plain launches for good.
    // ORBX_NO_GRAPHS=1 switches the capture off: while a stream captures (once per frame size, ~0.2 ms), a copy on the legacy stream
    // from ANY other thread fails with hipErrorStreamCaptureImplicit (tests/stress_threads.py met it in the FEM solver's former graph)
    // -- a host that cannot make its first two pairs before its other threads call into the library should set it.
    static const bool graphs_allowed = getenv("ORBX_NO_GRAPHS") == nullptr;
    const bool can = as_graph && graphs_allowed && ex->prof.mask == 0 && !ex->g_failed;
    if (can && ex->g_exec && ex->g_w == width && ex->g_h == height && ex->g_stride == stride) {
        ORBX_HIP(hipGraphLaunch(ex->g_exec, st));
        ex->last_batch = 1; ex->last_stream = st;
        return ORBX_OK;
    }
    const bool second = ex->g_seen_w == width && ex->g_seen_h == height && ex->g_seen_stride == stride;
    ex->g_seen_w = width; ex->g_seen_h = height; ex->g_seen_stride = stride;
    if (can && second && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        rc = enqueue();
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(st, &g);
        hipGraphExec_t x = nullptr;
        if (rc == ORBX_OK && e == hipSuccess && g && hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess) {
            drop_graph(ex);
            ex->g_graph = g; ex->g_exec = x; ex->g_w = width; ex->g_h = height; ex->g_stride = stride;
            ORBX_HIP(hipGraphLaunch(ex->g_exec, st));
            return ORBX_OK;
        }
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        ex->g_failed = true;        // nothing of the captured chain has run: enqueue it plainly
    }
    return enqueue();
}

static int extract_finish(orbx_extractor *ex, orbx_keypoint *kps, uint8_t *desc, int cap, int *n)
{
    ORBX_HIP(hipStreamSynchronize(ex->stream));
    const uint8_t *o = ex->h_pin + ex->pin_result_off;
    int cnt = 0;
    memcpy(&cnt, o, sizeof(int));
    *n = cnt;
    if (cnt > cap) ORBX_FAIL(ORBX_ERR_CAPACITY, "keypoint buffer too small");
    if (cnt > 0) {
        if (kps) memcpy(kps, o + 16, sizeof(orbx_keypoint) * cnt);
        if (desc) memcpy(desc, o + result_desc_off(ex), (size_t)32 * cnt);
    }
    return ORBX_OK;
}

int orbx_extract(orbx_extractor *ex, const uint8_t *image, int width, int height, int stride, orbx_keypoint *kps,
                 uint8_t *desc, int cap, int *n)
{
    if (!ex || !n) ORBX_FAIL(ORBX_ERR_ARG, "null argument");
    if (!image || width <= 0 || height <= 0) { *n = 0; return ORBX_OK; } // empty image: outputs untouched (:1054)
    const int rc = extract_enqueue(ex, image, width, height, stride);
    return rc != ORBX_OK ? rc : extract_finish(ex, kps, desc, cap, n);
}

int orbx_extract_pair(orbx_extractor *left, const uint8_t *image_left, orbx_extractor *right, const uint8_t *image_right, int width,
                      int height, int stride, orbx_keypoint *kps_left, uint8_t *desc_left, int cap_left, int *n_left,
                      orbx_keypoint *kps_right, uint8_t *desc_right, int cap_right, int *n_right)
{
    if (!left || !right || left == right || !n_left || !n_right || !image_left || !image_right || width <= 0 || height <= 0 || stride < width)
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    // both chains are on their queues before the host waits for either: the two extractions of a stereo frame overlap on the
    // device as they do on the reference's two threads (Frame.cc:78-81), without the threads
    int rc = extract_enqueue(left, image_left, width, height, stride, true);
    if (rc == ORBX_OK) rc = extract_enqueue(right, image_right, width, height, stride, true);
    if (rc != ORBX_OK) { (void)hipStreamSynchronize(left->stream); return rc; }
    rc = extract_finish(left, kps_left, desc_left, cap_left, n_left);
    const int rc2 = extract_finish(right, kps_right, desc_right, cap_right, n_right);
    return rc != ORBX_OK ? rc : rc2;
}

int orbx_result_dev(orbx_extractor *ex, const orbx_keypoint **kps, const uint8_t **desc, const int32_t **counts, int *capacity)
{
    if (!ex || !ex->d_kps) ORBX_FAIL(ORBX_ERR_ARG, "no results");
    if (kps) *kps = ex->d_kps;
    if (desc) *desc = ex->d_desc;
    if (counts) *counts = ex->d_counts;
    if (capacity) *capacity = ex->kcap;
    return ORBX_OK;
}

int orbx_copy_results_dev(orbx_extractor *ex, orbx_keypoint *kps_dst, uint8_t *desc_dst, int32_t *counts_dst, void *stream_)
{
    if (!ex || !ex->d_kps || ex->last_batch <= 0) ORBX_FAIL(ORBX_ERR_ARG, "no results");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : ex->stream;
    const size_t B = (size_t)ex->last_batch;
    if (kps_dst) ORBX_HIP(hipMemcpyAsync(kps_dst, ex->d_kps, sizeof(orbx_keypoint) * ex->kcap * B, hipMemcpyDefault, st));
    if (desc_dst) ORBX_HIP(hipMemcpyAsync(desc_dst, ex->d_desc, (size_t)32 * ex->kcap * B, hipMemcpyDefault, st));
    if (counts_dst) ORBX_HIP(hipMemcpyAsync(counts_dst, ex->d_counts, sizeof(int) * B, hipMemcpyDefault, st));
    return ORBX_OK;
}

static int copy_level(orbx_extractor *ex, const uint8_t *buf, int frame, int level, uint8_t *out, int out_stride, int padded)
{
    if (!ex || !out || frame < 0 || frame >= ex->last_batch || level < 0 || level >= ex->nlevels)
        ORBX_FAIL(ORBX_ERR_ARG, "bad frame/level");
    const LevelInfo &lv = ex->lv[level];
    const int w = padded ? lv.w + 2 * EDGE : lv.w, h = padded ? lv.h + 2 * EDGE : lv.h;
    if (out_stride < w) ORBX_FAIL(ORBX_ERR_ARG, "out_stride too small");
    const uint8_t *src = buf + (size_t)frame * ex->frame_bytes + lv.off +
                         (padded ? (size_t)(PADX - EDGE) : (size_t)EDGE * lv.stride + PADX);
    ORBX_HIP(hipMemcpy2DAsync(out, out_stride, src, lv.stride, w, h, hipMemcpyDeviceToHost, ex->last_stream));
    ORBX_HIP(hipStreamSynchronize(ex->last_stream));
    return ORBX_OK;
}

int orbx_pyramid_level(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride)
{ return copy_level(ex, ex ? ex->d_pyr : nullptr, frame, level, out, out_stride, 0); }
int orbx_pyramid_level_padded(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride)
{ return copy_level(ex, ex ? ex->d_pyr : nullptr, frame, level, out, out_stride, 1); }
int orbx_debug_blurred_level(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride)
{
    // the blurred buffer is laid out in strips (orbx_internal.h): the level's strips come over whole and are put back into rows here
    if (!ex || !ex->d_blur || frame < 0 || frame >= ex->last_batch || level < 0 || level >= ex->nlevels || !out)
        ORBX_FAIL(ORBX_ERR_ARG, "bad frame/level");
    const LevelInfo &lv = ex->lv[level];
    if (out_stride < lv.w) ORBX_FAIL(ORBX_ERR_ARG, "out_stride too small");
    const int nstrips = lv.stride / 16, bcol = ex->bcol[level];
    std::vector<uint8_t> strips((size_t)nstrips * bcol);
    ORBX_HIP(hipMemcpyAsync(strips.data(), ex->d_blur + (size_t)frame * ex->blur_frame_bytes + ex->boff[level], strips.size(),
                            hipMemcpyDeviceToHost, ex->last_stream));
    ORBX_HIP(hipStreamSynchronize(ex->last_stream));
    for (int y = 0; y < lv.h; ++y)
        for (int x = 0; x < lv.w; ++x) {
            const int X = PADX + x;
            out[(size_t)y * out_stride + x] = strips[(size_t)(X >> 4) * bcol + (size_t)(y + EDGE) * 16 + (X & 15)];
        }
    return ORBX_OK;
}

int orbx_debug_level_candidates(orbx_extractor *ex, int frame, int level, float *xyr, int cap, int *n)
{
    if (!ex || frame < 0 || frame >= ex->last_batch || level < 0 || level >= ex->nlevels || !n)
        ORBX_FAIL(ORBX_ERR_ARG, "bad frame/level");
    hipStream_t st = ex->last_stream;
    int M = 0;
    ORBX_HIP(hipMemcpyAsync(&M, ex->d_level_ncand + frame * ex->nlevels + level, sizeof(int), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    *n = M;
    if (M > cap) ORBX_FAIL(ORBX_ERR_CAPACITY, "candidate buffer too small");
    std::vector<uint32_t> pk(M > 0 ? M : 1);
    if (M > 0) {
        ORBX_HIP(hipMemcpyAsync(pk.data(), ex->d_kpos + (size_t)frame * ex->keys_per_frame + ex->lv[level].key_base,
                                sizeof(uint32_t) * M, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
    }
    for (int i = 0; i < M; i++) {
        xyr[3 * i] = (float)((pk[i] >> 8) & 0xfffu);
        xyr[3 * i + 1] = (float)(pk[i] >> 20);
        xyr[3 * i + 2] = (float)(pk[i] & 0xffu);
    }
    return ORBX_OK;
}

int orbx_debug_level_keypoints(orbx_extractor *ex, int frame, int level, orbx_keypoint *kps, int cap, int *n)
{
    if (!ex || frame < 0 || frame >= ex->last_batch || level < 0 || level >= ex->nlevels || !n)
        ORBX_FAIL(ORBX_ERR_ARG, "bad frame/level");
    hipStream_t st = ex->last_stream;
    std::vector<int> lc(ex->nlevels);
    ORBX_HIP(hipMemcpyAsync(lc.data(), ex->d_level_count + frame * ex->nlevels, sizeof(int) * ex->nlevels, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    int first = 0;
    for (int l = 0; l < level; l++) first += lc[l];
    const int cnt = lc[level];
    *n = cnt;
    if (cnt > cap) ORBX_FAIL(ORBX_ERR_CAPACITY, "keypoint buffer too small");
    if (cnt == 0) return ORBX_OK;
    std::vector<uint32_t> pk(cnt);
    ORBX_HIP(hipMemcpyAsync(pk.data(), ex->d_sel + (size_t)frame * ex->sel_per_frame + ex->lv[level].sel_base,
                            sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(kps, ex->d_kps + (size_t)frame * ex->kcap + first, sizeof(orbx_keypoint) * cnt, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < cnt; i++) { // level coordinates, before pt *= scale
        kps[i].x = (float)((pk[i] >> 8) & 0xfffu) + MIN_BORDER;
        kps[i].y = (float)(pk[i] >> 20) + MIN_BORDER;
    }
    return ORBX_OK;
}

} // extern "C"
