// orbm_pnp.hip -- PnPsolver (src/PnPsolver.cc) on the device: every EPnP RANSAC hypothesis of up to 64 candidate keyframes in one call.
//
// An iteration of PnPsolver::iterate draws its four indices from a freshly reset list (:193-206) and reads no other iteration's
// result: the caller draws the sets of all iterations first, orbm_pnp_hypotheses evaluates compute_pose (:938-986) and CheckInliers
// (:763-794) for each, marks the hypotheses that set a new best with at least min_inliers, runs Refine (:649-694) on those, and what
// iterate returns is a fold over the results that the caller runs on the host (include/orbslam_hip.hpp, orb_slam2_e_amd/pnp.py).
// Three launches on one leased workspace's stream, one staged upload, one host wait:
//   k_pnp_hypotheses   one wave per (problem, hypothesis): EPnP of the four correspondences through orbm_epnp.h, whose work arrays
//                      (the 12 x 12 MtM / Ut among them) are in LDS, not in registers: the per-lane-redundant scheme of
//                      k_sim3_hypotheses would need 288 doubles per lane for that matrix alone.  Lane k owns element k of a row in
//                      the Jacobi rotations and the products of the ordered sums, one output element in the sums over the
//                      correspondences; what is left runs in every lane on the same values.  Then the lanes stride over the n
//                      correspondences; __ballot words are the mask, their popcounts the count.
//   k_pnp_records      one wave per problem: walks the H counts in order and marks the records.
//   k_pnp_refine       one wave per (problem, hypothesis); non-records clear their outputs and leave.  Every sum over the inliers
//                      is one sequential double chain in index order, owned by one lane; the inliers are read off the hypothesis'
//                      mask, and nothing is stored per correspondence (orbm_epnp.h), so a Refine set has no size limit of its own.
// Records behind the one whose Refine succeeds are speculative: the fold never reads them; they cost device time only.
// No float or double atomics; every sum has a fixed order; -ffp-contract=off; nothing transcendental.
#include <atomic>

#include "orbm_epnp.h"
#include "orbm_internal.h"

using namespace orbm_detail;

namespace {

constexpr int PNP_MAX_P = 64, PNP_MAX_N = 8192, PNP_MAX_H = 1024, PNP_DEBUG_MAX_N = 2048;

// One problem of a call, staged with the inputs.  o_*: byte offsets in the workspace.
struct PnpDev {
    unsigned o_Xw, o_uv, o_oct, o_sets;                               // staged inputs
    unsigned o_mask, o_rmask;                                         // results: [H][(n + 63) / 64] 64-bit words each
    int n, H, hyp0, min_inliers, best_in;                             // hyp0: index of the problem's first hypothesis in the call
    float th2;
    double fu, fv, uc, vc;
};

// orbm_epnp's work split on the device: element e belongs to lane e % 64 of the block's one wave
struct Wave {
    int lane;
    template <class F> __host__ __device__ __forceinline__ void each(int count, F f) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
        for (int e = lane; e < count; e += 64) f(e);
        __syncthreads();
#endif
    }
};

__device__ __forceinline__ int problem_of(const PnpDev *probs, int P, int g)
{
    int p = 0;
    for (int j = 1; j < P; ++j) if (probs[j].hyp0 <= g) p = j;        // hyp0 ascends; problems without hypotheses share their successor's
    return p;
}

// CheckInliers (:763-794) with the pose in LDS: lane = correspondence, 64 per round.  Returns mnInliersi (the same in every lane).
__device__ __forceinline__ int check_inliers(const PnpDev &d, const char *ws, const float *sigma2, const double *Rt, unsigned long long *mask, int lane)
{
    const float *Xw = reinterpret_cast<const float *>(ws + d.o_Xw), *uv = reinterpret_cast<const float *>(ws + d.o_uv);
    const int *oct = reinterpret_cast<const int *>(ws + d.o_oct);
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rt[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = Rt[9 + k];
    const int words = (d.n + 63) >> 6;
    int count = 0;
    for (int w = 0; w < words; ++w) {
        const int i = 64 * w + lane;
        bool in = false;
        if (i < d.n) {
            const float X[3] = {Xw[3 * i], Xw[3 * i + 1], Xw[3 * i + 2]}, p2d[2] = {uv[2 * i], uv[2 * i + 1]};
            in = orbm_epnp::check_inlier(R, t, X, p2d, d.fu, d.fv, d.uc, d.vc, sigma2[oct[i]] * d.th2);       // mvMaxError[i] (:158)
        }
        const unsigned long long word = __ballot(in);                 // bits past n are 0
        count += __popcll(word);
        if (lane == 0) mask[w] = word;
    }
    return count;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(const PnpDev *__restrict__ probs, int P, char *__restrict__ ws, const float *__restrict__ sigma2,
                                                       orbm_pnp_hypothesis *__restrict__ hyp)
{
    __shared__ orbm_epnp::Work wk;
    __shared__ double Rt[12];
    const int lane = threadIdx.x, g = blockIdx.x;
    const PnpDev &d = probs[problem_of(probs, P, g)];
    const int h = g - d.hyp0;
    orbm_epnp::Points pts;
    pts.Xw = reinterpret_cast<const float *>(ws + d.o_Xw); pts.uv = reinterpret_cast<const float *>(ws + d.o_uv);
    pts.sel = reinterpret_cast<const int32_t *>(ws + d.o_sets) + 4 * h;        // inside [0, n): checked on the host before the launch
    pts.N = 4; pts.count = 4;
    const double rep = orbm_epnp::compute_pose(Wave{lane}, wk, pts, d.fu, d.fv, d.uc, d.vc, Rt, Rt + 9);
    __syncthreads();
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(ws + d.o_mask) + (size_t)h * ((d.n + 63) >> 6);
    const int count = check_inliers(d, ws, sigma2, Rt, mask, lane);
    if (lane == 0) {
        orbm_pnp_hypothesis &o = hyp[g];
        for (int k = 0; k < 9; ++k) o.R[k] = Rt[k];
        for (int k = 0; k < 3; ++k) o.t[k] = Rt[9 + k];
        o.rep_error = rep;
        o.ninliers = count;
    }
}

__global__ __launch_bounds__(64) void k_pnp_records(const PnpDev *__restrict__ probs, orbm_pnp_hypothesis *__restrict__ hyp)
{
    const PnpDev &d = probs[blockIdx.x];
    if (threadIdx.x != 0) return;
    int best = d.best_in;                                             // mnBestInliers as the caller carries it
    for (int h = 0; h < d.H; ++h) {
        orbm_pnp_hypothesis &o = hyp[d.hyp0 + h];
        const int c = o.ninliers;
        const bool record = c >= d.min_inliers && c > best;          // :214, :218
        if (record) best = c;
        o.refined = record ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void k_pnp_refine(const PnpDev *__restrict__ probs, int P, char *__restrict__ ws, const float *__restrict__ sigma2,
                                                   orbm_pnp_hypothesis *__restrict__ hyp)
{
    __shared__ orbm_epnp::Work wk;
    __shared__ double Rt[12];
    const int lane = threadIdx.x, g = blockIdx.x;
    const PnpDev &d = probs[problem_of(probs, P, g)];
    const int h = g - d.hyp0, words = (d.n + 63) >> 6;
    orbm_pnp_hypothesis &o = hyp[g];
    unsigned long long *rmask = reinterpret_cast<unsigned long long *>(ws + d.o_rmask) + (size_t)h * words;
    if (!o.refined) {                                                 // the same in every lane
        for (int w = lane; w < words; w += 64) rmask[w] = 0;
        if (lane == 0) {
            for (int k = 0; k < 9; ++k) o.Rr[k] = 0.0;
            for (int k = 0; k < 3; ++k) o.tr[k] = 0.0;
            o.nrefined = 0; o.pad = 0;
        }
        return;
    }
    orbm_epnp::Points pts;
    pts.Xw = reinterpret_cast<const float *>(ws + d.o_Xw); pts.uv = reinterpret_cast<const float *>(ws + d.o_uv);
    pts.mask = reinterpret_cast<const uint64_t *>(ws + d.o_mask) + (size_t)h * words;   // mvbBestInliers = this hypothesis' flags
    pts.N = d.n; pts.count = o.ninliers;
    orbm_epnp::compute_pose(Wave{lane}, wk, pts, d.fu, d.fv, d.uc, d.vc, Rt, Rt + 9);
    __syncthreads();
    const int count = check_inliers(d, ws, sigma2, Rt, rmask, lane);
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) o.Rr[k] = Rt[k];
        for (int k = 0; k < 3; ++k) o.tr[k] = Rt[9 + k];
        o.nrefined = count; o.pad = 0;
    }
}

std::atomic<int> g_last_pnp_waits{0};      // host waits of the last orbm_pnp_hypotheses call of this process

} // namespace

extern "C" {

int orbm_pnp_hypotheses(const orbm_pnp_problem *problems, int P, const float *level_sigma2, int nlevels, const int32_t *best_in,
                        orbm_pnp_hypothesis *hyp, void *inliers, void *refined_inliers)
{
    g_last_pnp_waits.store(0, std::memory_order_relaxed);
    if (P < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (P > PNP_MAX_P) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 64 problems in one call");
    if (P && !problems) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    int total = 0;
    for (int p = 0; p < P; ++p) {
        const orbm_pnp_problem &q = problems[p];
        if (q.n < 0 || q.H < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        if (q.n > PNP_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 correspondences in a problem");
        if (q.H > PNP_MAX_H) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 1,024 hypotheses in a problem");
        if (q.H == 0) continue;
        if (q.n < 4) ORBX_FAIL(ORBX_ERR_ARG, "a hypothesis needs four correspondences");
        if (q.min_inliers < 1) ORBX_FAIL(ORBX_ERR_ARG, "min_inliers must be at least 1");
        if (!q.Xw || !q.uv || !q.octave || !q.sets || !level_sigma2 || nlevels < 1 || !hyp || !inliers || !refined_inliers)
            ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        for (int i = 0; i < 4 * q.H; ++i)
            if (q.sets[i] < 0 || q.sets[i] >= q.n) ORBX_FAIL(ORBX_ERR_ARG, "set index out of range");
        for (int i = 0; i < q.n; ++i)
            if (q.octave[i] < 0 || q.octave[i] >= nlevels) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
        total += q.H;
    }
    if (total == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    std::vector<PnpDev> dev((size_t)P);
    StagedCall sc;
    const size_t o_dev = sc.in(dev.data(), sizeof(PnpDev) * (size_t)P), o_sg = sc.in(level_sigma2, sizeof(float) * (size_t)nlevels);
    int h0 = 0;
    for (int p = 0; p < P; ++p) {
        const orbm_pnp_problem &q = problems[p];
        PnpDev &d = dev[p];
        memset(&d, 0, sizeof(d));
        d.n = q.n; d.H = q.H; d.hyp0 = h0; d.min_inliers = q.min_inliers; d.best_in = best_in ? best_in[p] : 0;
        d.th2 = q.th2; d.fu = q.fu; d.fv = q.fv; d.uc = q.uc; d.vc = q.vc;
        h0 += q.H;
        if (q.H == 0) continue;
        const size_t n = (size_t)q.n;
        d.o_Xw = (unsigned)sc.in(q.Xw, sizeof(float) * 3 * n); d.o_uv = (unsigned)sc.in(q.uv, sizeof(float) * 2 * n);
        d.o_oct = (unsigned)sc.in(q.octave, sizeof(int32_t) * n); d.o_sets = (unsigned)sc.in(q.sets, sizeof(int32_t) * 4 * (size_t)q.H);
    }
    const size_t o_hyp = sc.out(sizeof(orbm_pnp_hypothesis) * (size_t)total);
    for (int p = 0; p < P; ++p) {
        PnpDev &d = dev[p];
        if (d.H == 0) continue;
        const size_t bytes = sizeof(uint64_t) * (size_t)d.H * (size_t)((d.n + 63) / 64);
        d.o_mask = (unsigned)sc.out(bytes); d.o_rmask = (unsigned)sc.out(bytes);
    }
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)total), dim3(64), 0, sc.stream(), sc.d<const PnpDev>(o_dev), P, sc.d<char>(0),
                       sc.d<const float>(o_sg), sc.d<orbm_pnp_hypothesis>(o_hyp));
    ORBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_records, dim3((unsigned)P), dim3(64), 0, sc.stream(), sc.d<const PnpDev>(o_dev), sc.d<orbm_pnp_hypothesis>(o_hyp));
    ORBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)total), dim3(64), 0, sc.stream(), sc.d<const PnpDev>(o_dev), P, sc.d<char>(0),
                       sc.d<const float>(o_sg), sc.d<orbm_pnp_hypothesis>(o_hyp));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_pnp_waits.store(sc.waits, std::memory_order_relaxed);       // counted where the stream is waited for
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(hyp, sc.r<orbm_pnp_hypothesis>(o_hyp), sizeof(orbm_pnp_hypothesis) * (size_t)total);
    uint64_t *out = static_cast<uint64_t *>(inliers), *rout = static_cast<uint64_t *>(refined_inliers);
    for (int p = 0; p < P; ++p) {
        const PnpDev &d = dev[p];
        const size_t words = (size_t)d.H * (size_t)((d.n + 63) / 64);
        if (d.H) {
            memcpy(out, sc.r<uint64_t>(d.o_mask), sizeof(uint64_t) * words);
            memcpy(rout, sc.r<uint64_t>(d.o_rmask), sizeof(uint64_t) * words);
        }
        out += words; rout += words;
    }
    return ORBX_OK;
}

int orbm_debug_last_pnp_waits(void) { return g_last_pnp_waits.load(std::memory_order_relaxed); }

int orbm_debug_pnp_pose(const double *pws, const double *us, int n, const double *fu_fv_uc_vc, double *R, double *t, double *rep_error)
{
    if (!pws || !us || !fu_fv_uc_vc || !R || !t || !rep_error) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n < 4) ORBX_FAIL(ORBX_ERR_ARG, "EPnP needs four correspondences");
    if (n > PNP_DEBUG_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 2,048 correspondences");
    orbm_epnp::Work wk;
    orbm_epnp::Points pts;
    pts.pwd = pws; pts.usd = us; pts.N = n; pts.count = n;
    *rep_error = orbm_epnp::compute_pose(orbm_epnp::Serial(), wk, pts, fu_fv_uc_vc[0], fu_fv_uc_vc[1], fu_fv_uc_vc[2], fu_fv_uc_vc[3], R, t);
    return ORBX_OK;
}

} // extern "C"
