// orbm_refine_sim3.hip -- the refinement tail of LoopClosing::ComputeSim3 (src/LoopClosing.cc:311-341) for up to 64 attempts against
// one current keyframe in ONE call: SearchBySim3 (src/ORBmatcher.cc:1303-1527), the correspondence walk of OptimizeSim3
// (src/Optimizer.cc:1483-1520) and OptimizeSim3 itself (:1564-1624), one staged upload, four launches, one host wait.
//   1. k_project_pair_jobs (orbm_search.hip): both projection prefixes of every attempt, job = (attempt, direction);
//   2. k_win_best_jobs (orbm_window.hip): both window searches of every attempt;
//   3. k_refine_gather (here): the agreement check, then the walk of Optimizer.cc:1483-1520 -- one workgroup per attempt compacts the
//      correspondences in ascending i1 with a prefix scan (no atomics: the optimiser's sums depend on the pair order) and fills the
//      problem's arrays and its n;
//   4. k_sim3_optimize (orbm_sim3opt.hip), as it is, over the device-built problems.
// vbAlreadyMatched1 / 2 (:1333-1343) are derived from the seeds on the host, while the inputs are staged.  The scatter back through
// the compact-to-i1 list (vpMatches1 as OptimizeSim3 leaves it) is host work behind the wait.  Every device loop is bounded by a
// count the host checked; no workgroup waits for another.
#include <limits.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "orbm_internal.h"
#include "orbm_search_internal.h"
#include "orbm_sim3opt_internal.h"

using namespace orbm_detail;

namespace {

constexpr int RG_T = 1024;              // threads of a gather workgroup: a chunk is a round of dependent loads (seed, valid, position, keypoint), so few chunks

// One attempt of a call, staged with the inputs.  o_*: byte offsets in the workspace.
struct RefineDev {
    unsigned o_seed, o_valid2, o_pos2, o_inv2;          // staged: seed12 [n1]; points2.valid [n2], pos [n2][3]; kf2's sorted position by keypoint [n2]
    unsigned o_best1, o_idx1, o_best2, o_idx2;          // the two window searches' results [n1] / [n2]
    unsigned o_found, o_list, o_cnt;                    // results: found12 [n1], the compact-to-i1 list [n1], {nfound, n}
    int n2;
    const SeqKp *kp2;                                   // kf2's keypoints in sorted order (mvKeysUn: position, octave)
};
struct RefineShared {
    unsigned o_valid1, o_pos1, o_inv1;
    int n1, th_high;
    const SeqKp *kp1;
};

// The agreement check of SearchBySim3 (:1509-1524) and the walk of OptimizeSim3 (Optimizer.cc:1483-1520) of attempt blockIdx.x:
// i2 = the seed, else what the search found; (i1, i2) is a correspondence iff i2 >= 0 and both map points are valid (non-NULL, not
// bad).  Chunks of RG_T keypoints in order, a running base between them: pair k of the problem is the k-th correspondence by i1.
__global__ __launch_bounds__(RG_T) void k_refine_gather(const RefineDev *__restrict__ attempts, Sim3OptDev *__restrict__ probs,
                                                        char *__restrict__ ws, RefineShared sh)
{
    constexpr int NW = RG_T / 64;
    __shared__ int s_pairs[NW], s_found[NW];
    const RefineDev &a = attempts[blockIdx.x];
    Sim3OptDev &d = probs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n1 = sh.n1, n2 = a.n2;
    const int *seed = reinterpret_cast<const int *>(ws + a.o_seed);
    const int *best1 = reinterpret_cast<const int *>(ws + a.o_best1), *idx1 = reinterpret_cast<const int *>(ws + a.o_idx1);
    const int *best2 = reinterpret_cast<const int *>(ws + a.o_best2), *idx2 = reinterpret_cast<const int *>(ws + a.o_idx2);
    const uint8_t *valid1 = reinterpret_cast<const uint8_t *>(ws + sh.o_valid1), *valid2 = reinterpret_cast<const uint8_t *>(ws + a.o_valid2);
    const float *pos1 = reinterpret_cast<const float *>(ws + sh.o_pos1), *pos2 = reinterpret_cast<const float *>(ws + a.o_pos2);
    const int *inv1 = reinterpret_cast<const int *>(ws + sh.o_inv1), *inv2 = reinterpret_cast<const int *>(ws + a.o_inv2);
    int *found12 = reinterpret_cast<int *>(ws + a.o_found), *list = reinterpret_cast<int *>(ws + a.o_list);
    float *X1 = reinterpret_cast<float *>(ws + d.o_X1w), *X2 = reinterpret_cast<float *>(ws + d.o_X2w);
    float *ob1 = reinterpret_cast<float *>(ws + d.o_obs1), *ob2 = reinterpret_cast<float *>(ws + d.o_obs2);
    int *oc1 = reinterpret_cast<int *>(ws + d.o_oct1), *oc2 = reinterpret_cast<int *>(ws + d.o_oct2);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int base = 0, nfound = 0;
    for (int c0 = 0; c0 < n1; c0 += RG_T) {
        const int i1 = c0 + tid;
        int i2 = -1;
        bool found = false, pair = false;
        if (i1 < n1) {
            int f = -1;
            if (n2 > 0) {       // (an attempt without keypoints in KF2 searched nothing: its result arrays were never written)
                const int v = sim3_accepted(best1[i1], idx1[i1], sh.th_high);
                found = sim3_agreed(i1, v, best2, idx2, n2, sh.th_high);
                if (found) f = v;
            }
            found12[i1] = f;
            const int s = seed[i1];
            i2 = s >= 0 ? s : f;                                    // (a seed of -2 blocked the slot in the search: f is -1)
            pair = i2 >= 0 && valid1[i1] && valid2[i2];             // seeds lie inside [-2, n2): checked on the host
        }
        const unsigned long long bp = __ballot(pair), bf = __ballot(found);
        if (lane == 0) { s_pairs[wave] = __popcll(bp); s_found[wave] = __popcll(bf); }
        __syncthreads();
        int off = base + __popcll(bp & lt);
        _Pragma("unroll") for (int w = 0; w < NW; ++w) {
            if (w < wave) off += s_pairs[w];
            base += s_pairs[w];
            nfound += s_found[w];
        }
        if (pair) {
            const SeqKp k1 = sh.kp1[inv1[i1]], k2 = a.kp2[inv2[i2]];
            _Pragma("unroll") for (int k = 0; k < 3; ++k) { X1[3 * off + k] = pos1[3 * i1 + k]; X2[3 * off + k] = pos2[3 * i2 + k]; }
            ob1[2 * off] = k1.x; ob1[2 * off + 1] = k1.y; ob2[2 * off] = k2.x; ob2[2 * off + 1] = k2.y;
            oc1[off] = k1.octave; oc2[off] = k2.octave;             // inside [0, nlevels): the handles' octave ranges, checked on the host
            list[off] = i1;
        }
        __syncthreads();                                            // the next chunk rewrites s_pairs / s_found
    }
    if (tid == 0) {
        d.n = base;
        int *cnt = reinterpret_cast<int *>(ws + a.o_cnt);
        cnt[0] = nfound; cnt[1] = base;
    }
}

std::atomic<int> g_last_refine_sim3_waits{0};  // host waits of the last orbm_refine_sim3_candidates call of this process

FrameView resident_view(const orbm_frame *f) { return {f->kp, f->desc, f->angle, f->perm, f->cell_off, f->gp}; }

// the keypoints' octaves name a pyramid level (inv_level_sigma2 is indexed with them) and fit a candidate entry's four bits
bool octaves_outside(const orbm_frame *f, int nlevels) { return f->n && (f->min_octave < 0 || f->max_octave >= nlevels || bad_octaves(f)); }

} // namespace

extern "C" {

int orbm_refine_sim3_candidates(const orbm_frame *kf1, const orbm_points *points1, const float *T1w, const orbm_view *view,
                                const float *inv_level_sigma2, const orbm_refine_sim3_attempt *attempts, int P, float th, int th_high,
                                float th2, int fix_scale, int32_t *nfound, orbm_sim3_opt_result *results)
{
    g_last_refine_sim3_waits.store(0, std::memory_order_relaxed);
    if (P < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (P > SO_MAX_P) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 64 attempts in one call");
    if (P == 0) return ORBX_OK;
    if (!kf1 || bad_view(view) || !T1w || !inv_level_sigma2 || !attempts || !nfound || !results ||
        bad_points(points1, true, false, false, view->nlevels) || points1->n != kf1->n)
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    const int n1 = kf1->n, nlevels = view->nlevels;
    if (n1 > SO_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in a keyframe");
    if (octaves_outside(kf1, nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    int n2max = 0;
    for (int p = 0; p < P; ++p) {
        const orbm_refine_sim3_attempt &q = attempts[p];
        if (!q.kf2 || !q.T2w || bad_points(q.points2, true, false, false, nlevels) || q.points2->n != q.kf2->n ||
            (n1 && (!q.found12 || !q.matches12)))
            ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        if (q.kf2->n > SO_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in a keyframe");
        if (octaves_outside(q.kf2, nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
        for (int i = 0; i < n1 && q.seed12; ++i)
            if (q.seed12[i] >= q.kf2->n || q.seed12[i] < -2) ORBX_FAIL(ORBX_ERR_ARG, "a seed names no keypoint of its keyframe");
        n2max = std::max(n2max, q.kf2->n);
    }
    const bool launches = n1 > 0 && n2max > 0;
    if (launches) ORBX_NEED_DEVICE();
    for (int p = 0; p < P; ++p) {               // what an attempt without a search and without a correspondence returns
        const orbm_refine_sim3_attempt &q = attempts[p];
        sim3_opt_empty_result(q.R12, q.t12, q.s12, results[p]);
        nfound[p] = 0;
        for (int i = 0; i < n1; ++i) { q.found12[i] = -1; q.matches12[i] = q.seed12 ? q.seed12[i] : -1; }
    }
    if (!launches) return ORBX_OK;

    // ---- the staged block: the records, the shared inputs, every attempt's inputs
    std::vector<PairSearchJob> jobs((size_t)2 * P);
    std::vector<RefineDev> att((size_t)P);
    std::vector<Sim3OptDev> dev((size_t)P);
    std::vector<std::vector<uint8_t>> seen1((size_t)P), seen2((size_t)P);     // valid with vbAlreadyMatched1 / 2 folded in
    const std::vector<int32_t> no_seed((size_t)n1, -1);
    const size_t m1 = (size_t)n1;
    StagedCall sc{};
    const size_t o_jobs = sc.in(jobs.data(), sizeof(PairSearchJob) * jobs.size()), o_att = sc.in(att.data(), sizeof(RefineDev) * att.size()),
                 o_dev = sc.in(dev.data(), sizeof(Sim3OptDev) * dev.size());
    const size_t o_sc = sc.in(view->scale_factors, sizeof(float) * (size_t)nlevels), o_sg = sc.in(inv_level_sigma2, sizeof(float) * (size_t)nlevels);
    const size_t o_desc1 = sc.in(points1->desc, 32 * m1), o_pos1 = sc.in(points1->pos, sizeof(float) * 3 * m1),
                 o_min1 = sc.in(points1->min_distance, sizeof(float) * m1), o_max1 = sc.in(points1->max_distance, sizeof(float) * m1);
    RefineShared sh;
    sh.o_valid1 = (unsigned)sc.in(points1->valid, m1); sh.o_pos1 = (unsigned)o_pos1;
    sh.o_inv1 = (unsigned)sc.in(kf1->inv_host.data(), sizeof(int) * m1);
    sh.n1 = n1; sh.th_high = th_high; sh.kp1 = kf1->kp;
    float R1[9], t1[3];
    pose_parts(T1w, R1, t1);
    for (int p = 0; p < P; ++p) {
        const orbm_refine_sim3_attempt &q = attempts[p];
        const orbm_points &pts2 = *q.points2;
        const int n2 = q.kf2->n;
        const size_t m2 = (size_t)n2;
        const int32_t *seed = q.seed12 ? q.seed12 : no_seed.data();
        RefineDev &a = att[p];
        Sim3OptDev &d = dev[p];
        PairSearchJob &j12 = jobs[2 * p], &j21 = jobs[2 * p + 1];
        memset(&a, 0, sizeof(a)); memset(&d, 0, sizeof(d)); memset(&j12, 0, sizeof(j12)); memset(&j21, 0, sizeof(j21));
        a.n2 = n2; a.kp2 = q.kf2->kp;
        a.o_seed = (unsigned)sc.in(seed, sizeof(int32_t) * m1);
        d.fix_scale = fix_scale ? 1 : 0; d.th2 = th2; d.s12 = q.s12;    // d.n: k_refine_gather's
        memcpy(d.R12, q.R12, sizeof(d.R12)); memcpy(d.t12, q.t12, sizeof(d.t12));
        memcpy(d.R1, R1, sizeof(R1)); memcpy(d.t1, t1, sizeof(t1));
        pose_parts(q.T2w, d.R2, d.t2);
        d.cam1[0] = d.cam2[0] = view->fx; d.cam1[1] = d.cam2[1] = view->fy; d.cam1[2] = d.cam2[2] = view->cx; d.cam1[3] = d.cam2[3] = view->cy;
        if (n2 == 0) continue;                  // nothing to search and no seed >= 0: the gather finds no pair, the optimiser returns the start
        // :1333-1343: a seeded slot of KF1 is not searched from, nor is the KF2 keypoint a seed names
        std::vector<uint8_t> &v1 = seen1[p], &v2 = seen2[p];
        v1.assign(points1->valid, points1->valid + m1); v2.assign(pts2.valid, pts2.valid + m2);
        for (int i = 0; i < n1; ++i)
            if (seed[i] != -1) { v1[i] = 0; if (seed[i] >= 0) v2[seed[i]] = 0; }
        a.o_valid2 = (unsigned)sc.in(pts2.valid, m2); a.o_pos2 = (unsigned)sc.in(pts2.pos, sizeof(float) * 3 * m2);
        a.o_inv2 = (unsigned)sc.in(q.kf2->inv_host.data(), sizeof(int) * m2);
        form_pair_cams(j12.cam, j21.cam, view, kf1, q.kf2, T1w, q.T2w, q.s12, q.R12, q.t12, th);
        j12.frame = resident_view(q.kf2); j21.frame = resident_view(kf1);
        j12.nq = n1; j21.nq = n2;
        j12.o_valid = (unsigned)sc.in(v1.data(), m1); j12.o_pos = (unsigned)o_pos1; j12.o_min = (unsigned)o_min1; j12.o_max = (unsigned)o_max1;
        j12.o_desc = (unsigned)o_desc1;
        j21.o_valid = (unsigned)sc.in(v2.data(), m2); j21.o_pos = a.o_pos2; j21.o_min = (unsigned)sc.in(pts2.min_distance, sizeof(float) * m2);
        j21.o_max = (unsigned)sc.in(pts2.max_distance, sizeof(float) * m2); j21.o_desc = (unsigned)sc.in(pts2.desc, 32 * m2);
    }
    // ---- scratch: queries and search results, the device-built problems (sized for n1 pairs)
    for (int p = 0; p < P; ++p) {
        RefineDev &a = att[p];
        Sim3OptDev &d = dev[p];
        const size_t m2 = (size_t)a.n2;
        if (m2) {
            jobs[2 * p].o_q = (unsigned)sc.scratch(sizeof(WinQuery) * m1); jobs[2 * p + 1].o_q = (unsigned)sc.scratch(sizeof(WinQuery) * m2);
            a.o_best1 = jobs[2 * p].o_best = (unsigned)sc.scratch(sizeof(int) * m1); a.o_idx1 = jobs[2 * p].o_idx = (unsigned)sc.scratch(sizeof(int) * m1);
            a.o_best2 = jobs[2 * p + 1].o_best = (unsigned)sc.scratch(sizeof(int) * m2); a.o_idx2 = jobs[2 * p + 1].o_idx = (unsigned)sc.scratch(sizeof(int) * m2);
        }
        d.o_X1w = (unsigned)sc.scratch(sizeof(float) * 3 * m1); d.o_X2w = (unsigned)sc.scratch(sizeof(float) * 3 * m1);
        d.o_obs1 = (unsigned)sc.scratch(sizeof(float) * 2 * m1); d.o_obs2 = (unsigned)sc.scratch(sizeof(float) * 2 * m1);
        d.o_oct1 = (unsigned)sc.scratch(sizeof(int) * m1); d.o_oct2 = (unsigned)sc.scratch(sizeof(int) * m1);
        if (n1 > SO_LDS_PAIRS) d.o_pair = (unsigned)sc.scratch(SO_PAIR_BYTES * (size_t)(n1 - SO_LDS_PAIRS));
    }
    // ---- results
    const size_t o_res = sc.out(sizeof(orbm_sim3_opt_result) * (size_t)P);
    for (int p = 0; p < P; ++p) {
        att[p].o_found = (unsigned)sc.out(sizeof(int) * m1); att[p].o_list = (unsigned)sc.out(sizeof(int) * m1);
        att[p].o_cnt = (unsigned)sc.out(2 * sizeof(int)); dev[p].o_kept = (unsigned)sc.out(m1);
    }
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipStream_t st = sc.stream();
    char *ws = sc.d<char>(0);
    const int max_nq = std::max(n1, n2max);
    launch_project_pair_jobs(st, sc.d<const PairSearchJob>(o_jobs), 2 * P, max_nq, ws, sc.d<const float>(o_sc));
    launch_win_best_jobs(st, sc.d<const PairSearchJob>(o_jobs), 2 * P, max_nq, ws);
    hipLaunchKernelGGL(k_refine_gather, dim3((unsigned)P), dim3(RG_T), 0, st, sc.d<const RefineDev>(o_att), sc.d<Sim3OptDev>(o_dev), ws, sh);
    launch_sim3_optimize(st, sc.d<const Sim3OptDev>(o_dev), P, ws, sc.d<const float>(o_sg), sc.d<orbm_sim3_opt_result>(o_res));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_refine_sim3_waits.store(sc.waits, std::memory_order_relaxed);   // counted where the stream is waited for
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(results, sc.r<orbm_sim3_opt_result>(o_res), sizeof(orbm_sim3_opt_result) * (size_t)P);
    for (int p = 0; p < P; ++p) {
        const orbm_refine_sim3_attempt &q = attempts[p];
        const int *cnt = sc.r<int>(att[p].o_cnt), *list = sc.r<int>(att[p].o_list);
        const uint8_t *kept = sc.r<uint8_t>(dev[p].o_kept);
        memcpy(q.found12, sc.r<int>(att[p].o_found), sizeof(int) * m1);
        nfound[p] = cnt[0];
        for (int i = 0; i < n1; ++i)
            if (q.matches12[i] == -1) q.matches12[i] = q.found12[i];        // (preset to the seeds above) :1513-1521
        const int n = std::min(std::max(cnt[1], 0), n1);
        for (int k = 0; k < n; ++k)                                         // :1577-1590 / :1611-1620 through vnIndexEdge
            if (!kept[k] && list[k] >= 0 && list[k] < n1) q.matches12[list[k]] = -1;
    }
    return ORBX_OK;
}

int orbm_debug_last_refine_sim3_waits(void) { return g_last_refine_sim3_waits.load(std::memory_order_relaxed); }

} // extern "C"
