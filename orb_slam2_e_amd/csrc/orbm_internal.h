// orbm_internal.h -- pieces shared by the matcher translation units (orbm_match.hip, orbm_frame.hip, orbm_window.hip,
// orbm_search.hip, orbm_triang.hip, orbm_pose.hip, orbm_pose_nr.hip, orbm_sim3.hip, orbm_sim3opt.hip, orbm_refine_sim3.hip, orbm_init.hip, orbm_pnp.hip, orbm_essential_graph.hip): the Frame grid
// constants, the keypoint / query records of the windowed searches, the resident frame (struct orbm_frame) and the map snapshot
// (struct orbm_map), the per-call workspace and small host / device helpers.  What only orbm_frame.hip, orbm_window.hip and
// orbm_search.hip share among themselves is in orbm_search_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/orbslam_hip.h"
#include "common.h"
#include "orbm_levenberg.h"
#include "orbx_math.h"

namespace orbm_detail {

constexpr int MT = 256; // threads per block of the small helper kernels
constexpr int FRAME_GRID_ROWS = 48, FRAME_GRID_COLS = 64; // include/Frame.h:37-38

struct WinQuery { float u, v, r, xr; int min_level, max_level; };
// Sorted keypoint record of the windowed searches: position sp in the array = rank in GetFeaturesInArea order.
struct SeqKp { float x, y, uright; int octave; };
struct GridParams { float min_x, min_y, inv_w, inv_h; };
struct FrameHdr { int n, ns, min_octave, max_octave; };     // what k_frame_build leaves in front of a resident frame's block
static_assert(sizeof(WinQuery) == sizeof(orbm_window_query), "query layout");

__device__ __forceinline__ int popc256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// cv::Mat gemm of one row of a 3 x 3 float matrix with a vector, plus t: the float row sum, then the sum with t in double.
__device__ __forceinline__ float gemm_row(const float *R, int r, float b0, float b1, float b2, float t)
{
    return (float)((double)(R[3 * r] * b0 + R[3 * r + 1] * b1 + R[3 * r + 2] * b2) + (double)t);
}

// ---- cv::Mat float arithmetic of the pose handling in front of the projection loops, on the host (a handful of operations
// per call; -ffp-contract=off keeps them unfused).  OpenCV 3.4 semantics restated (gemm's 3 x 3 special case: float row
// sum left to right, then float(double(sum) * alpha + double(c) * beta); scaling by a FLOAT factor with a + 0.0f).
inline void pose_parts(const float *T16, float *R, float *t)
{
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = T16[4 * r + c]; t[r] = T16[4 * r + 3]; }
}
inline void gemm3(const float *A, const float *b, double alpha, const float *c, double beta, float *d)
{
    float out[3];
    for (int k = 0; k < 3; ++k) {
        const float t = A[3 * k] * b[0] + A[3 * k + 1] * b[1] + A[3 * k + 2] * b[2];
        out[k] = (float)((double)t * alpha + (double)(c ? c[k] : 0.0f) * beta);
    }
    d[0] = out[0]; d[1] = out[1]; d[2] = out[2];
}
inline void transpose3(const float *A, float *At)
{
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) At[3 * r + c] = A[3 * c + r];
}
inline void scale_mat(const float *A, int n, double s, float *out)
{
    const float a = (float)s, b = (float)0.0;
    for (int i = 0; i < n; ++i) out[i] = A[i] * a + b;
}
inline void neg_Rt_t(const float *R, const float *t, float *out)   // -R.t() * t  (ORBmatcher.cc:1542, :1679, :504)
{
    float Rt[9];
    transpose3(R, Rt);
    gemm3(Rt, t, -1.0, nullptr, 0.0, out);
}

// The co-iteration of two FeatureVectors (ORBmatcher.cc:384-456, :745-828, :881-891 / :1004-1012), given as their ascending node
// ids: visit(a, b) for every node both hold (nodes1[a] == nodes2[b]); otherwise lower_bound on the other map.
template <class F>
inline void for_each_common_node(const int32_t *nodes1, int nn1, const int32_t *nodes2, int nn2, F visit)
{
    for (int a = 0, b = 0; a < nn1 && b < nn2;) {
        if (nodes1[a] == nodes2[b]) {
            visit(a, b);
            ++a; ++b;
        } else if (nodes1[a] < nodes2[b]) {
            while (a < nn1 && nodes1[a] < nodes2[b]) ++a;
        } else {
            while (b < nn2 && nodes2[b] < nodes1[a]) ++b;
        }
    }
}
// every feature index of a FeatureVector (off, items; nn nodes) names one of n features: 0, else -1
inline int bow_check_items(const int32_t *off, const int32_t *items, int nn, int n)
{
    for (int k = 0; k < (nn ? off[nn] : 0); ++k)
        if (items[k] < 0 || items[k] >= n) return -1;
    return 0;
}

// ---- the rotation-consistency check of every ORBmatcher search, one definition each for the device and the host code
constexpr int HISTO_LENGTH = 30;   // ORBmatcher.cc:40

// Bin of an angle difference angle1 - angle2 in the rotation histogram (e.g. ORBmatcher.cc:108-115, :994-1001).  Keypoint
// angles lie in [0, 360): the result is 0 .. HISTO_LENGTH - 1 (the reference asserts it; callers that take angles from outside
// check the range).
__host__ __device__ __forceinline__ int rotation_bin(float rot)
{
    const float factor = 1.0f / HISTO_LENGTH;
    if (rot < 0.0f) rot += 360.0f;
    const int bin = (int)roundf(rot * factor);
    return bin == HISTO_LENGTH ? 0 : bin;
}

// ORBmatcher::ComputeThreeMaxima (:1802-1843): keep[0..2] = the bins of the three largest counts (first wins a tie), the second
// and third only if they reach 10 % of the largest; -1 = none.
__host__ __device__ __forceinline__ void three_maxima(const int *hist, int *keep)
{
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
}

// The host tail of the SearchForTriangulation entry points (src/ORBmatcher.cc:992-1025): the rotation histogram over the matches
// (rot_of(i) = angle1 - angle2 of keypoint i's pair), ComputeThreeMaxima, rejection, and the count of what is left.
template <typename RotOf>
inline int triangulation_rotation_check(int32_t *match12, int n1, int check_orientation, RotOf rot_of, int *nmatches)
{
    if (check_orientation) {
        int hist[HISTO_LENGTH] = {0}, keep[3];
        std::vector<int> bin((size_t)n1, -1);
        for (int i = 0; i < n1; ++i)
            if (match12[i] >= 0) {
                const int b = rotation_bin(rot_of(i));
                if (b < 0 || b >= HISTO_LENGTH) ORBX_FAIL(ORBX_ERR_ARG, "keypoint angles outside [0, 360)");   // (the reference asserts)
                bin[i] = b; hist[b]++;
            }
        three_maxima(hist, keep);
        for (int i = 0; i < n1; ++i)
            if (bin[i] >= 0 && bin[i] != keep[0] && bin[i] != keep[1] && bin[i] != keep[2]) match12[i] = -1;
    }
    int nm = 0;
    for (int i = 0; i < n1; ++i) nm += match12[i] >= 0;
    *nmatches = nm;
    return ORBX_OK;
}

// Per-call scratch without per-call hipMalloc: a pool of workspaces (device arena, pinned
// host staging arena, a growable device buffer for candidate entries, a stream).  A call
// leases one, carves its arrays out of the arenas (staged inputs sit at the same offsets
// in both, so ONE copy uploads them) and releases the lease on return.  Concurrent
// callers (Tracking / LocalMapping / LoopClosing threads) get different workspaces.
// Workspaces live until process exit.
struct Workspace {
    char *dev = nullptr, *pin = nullptr;
    unsigned *ent = nullptr;
    size_t dev_cap = 0, pin_cap = 0, ent_cap = 0, used = 0;
    hipStream_t st = nullptr;
    unsigned gen = 0;    // call counter: a flag a kernel raises is this number, 1 .. 0x7ffffffe (0 is never a generation).  The arenas keep
                         // what earlier calls left: a word that is compared with the generation is WRITTEN by the call before it is read
                         // (staged as 0 with the inputs, or set either way by a kernel) -- stale memory may hold any number, this one included
    unsigned next_generation() const { return (gen % 0x7ffffffe) + 1; }    // the number the workspace's next call will use
    unsigned begin_generation() { return gen = next_generation(); }
    int reserve(size_t dev_bytes, size_t pin_bytes); // discards the contents
    int reserve_entries(size_t n);
    hipStream_t own_stream() { if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr; return st; }   // nullptr = failed (never hand out the legacy stream)
    size_t carve(size_t bytes) { const size_t o = used; used += (bytes + 255) & ~(size_t)255; return o; }
    template <typename T> T *d(size_t off) const { return reinterpret_cast<T *>(dev + off); }
    template <typename T> T *h(size_t off) const { return reinterpret_cast<T *>(pin + off); }
};
Workspace *workspace_acquire();
void workspace_release(Workspace *w);
// orbm_debug_fill_workspaces' share of orbm_frame.hip: every pooled (destroyed) frame block filled with `word` and waited for.
// Returns the number of blocks, -1 when a fill failed.
int frame_pool_fill(uint32_t word);
struct WorkspaceLease {
    Workspace *w;
    WorkspaceLease() : w(workspace_acquire()) {}
    ~WorkspaceLease() { workspace_release(w); }
};

// One host-array call: declare inputs (staged in pinned memory, uploaded with ONE copy), device scratch and outputs
// (downloaded with ONE copy), in that order; everything runs on the leased workspace's stream.
struct StagedCall {
    WorkspaceLease lease;
    Workspace &w;
    struct In { size_t off; const void *src; size_t bytes; };
    std::vector<In> ins;
    size_t staged = 0, res_off = 0, res_bytes = 0;
    int waits = 0;                  // host waits (stream synchronisations) of this call so far
    hipStream_t on = nullptr;       // set before upload(): run on this stream (a fem_model's) instead of the workspace's own
    StagedCall() : w(*lease.w) { w.used = 0; }
    size_t in(const void *src, size_t bytes)
    {
        const size_t o = w.carve(bytes ? bytes : 1);
        if (src && bytes) ins.push_back({o, src, bytes});
        staged = w.used;
        return o;
    }
    void in_at(size_t off, const void *src, size_t bytes) { if (src && bytes) ins.push_back({off, src, bytes}); } // inside an in(nullptr, n) block
    size_t scratch(size_t bytes) { return w.carve(bytes ? bytes : 1); }
    size_t out(size_t bytes)
    {
        if (!res_bytes) res_off = w.used;
        const size_t o = w.carve(bytes ? bytes : 1);
        res_bytes = w.used - res_off;
        return o;
    }
    bool offsets_fit_32_bits() const { return w.used <= 0xffffffffu; }  // for calls whose device records hold offsets as unsigned
    hipStream_t stream() const { return on ? on : w.st; }
    template <typename T> T *d(size_t off) const { return reinterpret_cast<T *>(w.dev + off); }
    template <typename T> const T *r(size_t off) const { return reinterpret_cast<const T *>(w.pin + (off - res_off)); }
    int upload() // after the last in / scratch / out
    {
        const char *dev_before = w.dev;
        if (w.reserve(w.used, staged > res_bytes ? staged : res_bytes)) return -1;
        if (on && w.dev != dev_before && hipStreamSynchronize(w.st) != hipSuccess) return -1;   // a grown arena is zeroed on the workspace's stream
        for (const In &i : ins) memcpy(w.pin + i.off, i.src, i.bytes);
        return orbx::stage_in(w.dev, w.pin, staged, stream()) != hipSuccess ? -1 : 0;
    }
    int download() { return download_head(res_bytes); }
    int download_head(size_t bytes) // the first bytes of the result block, in the middle of a call
    {
        if (orbx::stage_out(w.pin, w.dev + res_off, bytes, stream()) != hipSuccess) return -1;
        ++waits;
        return hipStreamSynchronize(stream()) == hipSuccess ? 0 : -1;
    }
};

// ---- OptimizationAlgorithmLevenberg::solve with the decisions on the host and the passes in kernels (orbm_ba.hip,
// orbm_essential_graph.hip).  Such a call's result block begins with the 128 bytes a trial reads back: 8 doubles, then 16 ints.
constexpr size_t LM_BLOCK_BYTES = 128;
enum { LM_SC_CHI2 = 0,              // chi2 at the iteration's start
       LM_SC_MAXDIAG = 3,           // the largest diagonal entry, and tau * that: computeLambdaInit (the bundle adjustments alone
       LM_SC_LAMBDA_INIT = 4,       // write these two and the two counts below; the essential graph leaves them untouched)
       LM_SC_TEMPCHI = 5,           // a trial's chi2
       LM_SC_SCALE = 6 };           // computeScale's sum
enum { LM_ISC_NACT = 0,             // the vertex poses of the round (the bundle adjustments)
       LM_ISC_OK2 = 1,              // the solve's verdict
       LM_ISC_NEDGES = 2 };         // the active edges of the round (the bundle adjustments)

struct LmNever { bool operator()() const { return false; } };

struct LmHostLoop {
    StagedCall &sc;
    orbm_ba_trial *log;             // [log_cap], or nullptr with log_cap 0
    int log_cap;
    LmStep lm;
    double currentChi = 0., iniChi = 0., rho = 0.;
    int qmax = 0, nt = 0;           // nt: trials of the call so far

    int read_block() { return sc.download_head(LM_BLOCK_BYTES); }
    double scalar(int k) const { return sc.r<double>(sc.res_off)[k]; }
    int flag(int k) const { return reinterpret_cast<const int *>(sc.r<double>(sc.res_off) + 8)[k]; }

    // The trial loop of one iteration (levenberg.cpp:129-226).  trial(lambda) enqueues a trial with its reductions and returns an
    // ORBX code; after_read() runs behind every read-back, in front of the verdict (a caller sets currentChi / iniChi, or lambda
    // itself, from the block there); pop() enqueues the copy back; terminate() is g2o's stop flag.  Every trial is appended to the
    // log.  Leaves rho and qmax for lm.end_iteration.
    template <class Trial, class AfterRead, class Pop, class Terminate = LmNever>
    int trials(int round, Trial &&trial, AfterRead &&after_read, Pop &&pop, Terminate &&terminate = Terminate())
    {
        iniChi = currentChi;
        rho = 0;
        qmax = 0;
        do {
            const int rc = trial(lm.lambda);
            if (rc != ORBX_OK) return rc;
            ORBX_HIP(hipGetLastError());
            if (read_block()) ORBX_FAIL(ORBX_ERR_HIP, "a trial's read-back failed");
            after_read();
            const bool ok2 = flag(LM_ISC_OK2) != 0;
            const double tempChi = ok2 ? scalar(LM_SC_TEMPCHI) : DBL_MAX;
            const LmVerdict vd = lm.verdict(currentChi, tempChi, ok2 ? scalar(LM_SC_SCALE) : 0.0, LmNothing(), pop);
            rho = vd.rho;
            if (nt < log_cap) {
                orbm_ba_trial &t = log[nt];
                t.tempChi = tempChi; t.currentChi = currentChi; t.rho = rho; t.lambda = lm.lambda; t.scale = vd.scale;
                t.round = round; t.qmax = qmax; t.accepted = vd.accepted ? 1 : 0; t.ok2 = ok2 ? 1 : 0;
            }
            ++nt;
            qmax++;
        } while (rho < 0 && qmax < 10 && !terminate());
        return ORBX_OK;
    }
};

// ---- the problems over two keyframes (orbm_sim3_problem / orbm_sim3_opt_problem, staged as Sim3Dev / Sim3OptDev): what the two
// public structs share has the same member names in both, and so have the two device records.

// every octave of both keyframes names a level
template <typename Problem>
inline bool octaves_in_range(const Problem &q, int nlevels)
{
    for (int i = 0; i < q.n; ++i)
        if (q.octave1[i] < 0 || q.octave1[i] >= nlevels || q.octave2[i] < 0 || q.octave2[i] >= nlevels) return false;
    return true;
}

// the points and octaves of both keyframes as staged inputs, Tcw1 / Tcw2 as R, t and the two cameras, into the device record
template <typename Problem, typename Dev>
inline void stage_two_keyframes(StagedCall &sc, const Problem &q, Dev &d)
{
    const size_t n = (size_t)q.n;
    d.o_X1w = (unsigned)sc.in(q.X1w, sizeof(float) * 3 * n); d.o_X2w = (unsigned)sc.in(q.X2w, sizeof(float) * 3 * n);
    d.o_oct1 = (unsigned)sc.in(q.octave1, sizeof(int32_t) * n); d.o_oct2 = (unsigned)sc.in(q.octave2, sizeof(int32_t) * n);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { d.R1[3 * r + c] = q.Tcw1[4 * r + c]; d.R2[3 * r + c] = q.Tcw2[4 * r + c]; }
        d.t1[r] = q.Tcw1[4 * r + 3]; d.t2[r] = q.Tcw2[4 * r + 3];
    }
    d.cam1[0] = q.fx1; d.cam1[1] = q.fy1; d.cam1[2] = q.cx1; d.cam1[3] = q.cy1;
    d.cam2[0] = q.fx2; d.cam2[1] = q.fy2; d.cam2[2] = q.cx2; d.cam2[3] = q.cy2;
}

// Work a caller appends to a whole-loop projection search, on the search's stream, behind the resolver and in front of the call's
// host wait (orbm_pose.hip: the pose solve of the tracking functions).  The driver (run_sequential, orbm_search.hip) asks the chain
// for its arrays while it lays the workspace out -- inputs inside the staged block (they travel with the call's one upload),
// results behind the search's result block (a result at offset o is read back at w.pin + (o - o_res)) -- and launches it once per
// attempt.  A search attempt may have to be repeated (see run_sequential); the flags that say so are only known on the device
// when the chain's kernel runs, so that kernel reads them itself and must leave at once if the attempt does not stand.
// collect() runs after the wait of the attempt that stands.
struct SearchChain {
    struct Ctx {
        const Workspace *w;
        hipStream_t st;
        const int *match_kp;        // [n], device: the resolver's result by keypoint index
        const int *flags;           // device: match count, (unused), "fixed point reached" (== gen), iterations
        const int *overflow;        // device: "a list outgrew its region" (== gen), staged as 0 with the call's inputs
        const uint8_t *qtakes;      // [nq], device: orbm_points::takes as staged (all 1 when the caller gave none)
        int n, nq, gen;
        bool check_overflow, check_converged;   // which of the two flags this attempt can raise
        size_t o_res;
    };
    int waits = 0;                  // host waits of the call so far
    bool launched = false;          // launch() ran in the attempt that stands
    virtual void carve_inputs(Workspace &w) = 0;
    virtual void fill_inputs(Workspace &w) = 0;
    virtual void carve_results(Workspace &w) = 0;
    virtual int launch(const Ctx &c) = 0;
    virtual void collect(const Ctx &c) = 0;
    virtual ~SearchChain() {}
};

// orbm_search_by_projection_last / orbm_search_by_projection_points with a chain (nullptr: the public functions)
int search_by_projection_last_chain(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const float *Tlw, const orbm_points *last,
                                    const uint8_t *occupied, float th, int mono, int th_high, int check_orientation, int32_t *match_kp,
                                    int32_t *match_q, int *nmatches, orbm_window_query *queries_out, SearchChain *chain);
int search_by_projection_points_chain(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *points,
                                      const uint8_t *occupied, float th, float viewing_cos_limit, int th_high, float nnratio,
                                      int32_t *match_kp, int32_t *match_q, int *nmatches, orbm_projected_point *projected_out,
                                      orbm_window_query *queries_out, SearchChain *chain);

} // namespace orbm_detail

// A frame resident in HBM: the sorted keypoint records, descriptors, angles, the permutation and the cell table of
// k_frame_build in ONE device block (recycled through a pool: a frame per image must not cost a hipMalloc), plus a host
// copy of the permutation (the per-call occupancy masks are given by keypoint index and staged in sorted order).
// Read-only after creation: any number of searches, from any thread, may use it at once.
struct orbm_frame {
    int n = 0, ns = 0, cap = 0, has_uright = 0;
    int nstereo = 0;                                        // keypoints with a right coordinate >= 0; -1: not known on the host (device arrays)
    int min_octave = 0, max_octave = -1;                    // over the keypoints (empty frame: 0, -1)
    float min_x = 0, min_y = 0, max_x = 0, max_y = 0;       // the bounds the SEARCHES use (cell range of a window, image tests)
    orbm_detail::GridParams gp = {0.f, 0.f, 0.f, 0.f};      // ... with the cell pitch the grid was built with
    char *block = nullptr;
    std::atomic<int> *refs = nullptr;                       // handles sharing the block (orbm_frame_alias)
    orbm_detail::SeqKp *kp = nullptr; uint4 *desc = nullptr; float *angle = nullptr; int *perm = nullptr, *cell_off = nullptr;
    orbm_detail::FrameHdr *hdr = nullptr;
    std::vector<int> perm_host;                             // [n]: keypoint index at sorted position (the first ns: inside the grid)
    std::vector<int> inv_host;                              // [n]: sorted position of keypoint index
};

// The map as the whole-map search reads it (orbm_map_create): descriptors, positions, normals and the two distance bounds of m
// map points in ONE device block.  Read-only after creation.
struct orbm_map {
    int m = 0;
    char *block = nullptr;
    uint4 *desc = nullptr; float *pos = nullptr, *nrm = nullptr, *mind = nullptr, *maxd = nullptr;
};
