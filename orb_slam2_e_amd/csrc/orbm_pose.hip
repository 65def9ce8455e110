// orbm_pose.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:264-476) as ONE launch: one workgroup per pose problem runs
// the 4 rounds, their Levenberg iterations and trials, the inlier / outlier classification between rounds and the final
// toCvMat, on g2o's code paths (Thirdparty/g2o/g2o: sparse_optimizer.cpp:425-504, optimization_algorithm_levenberg.cpp:63-267,
// base_unary_edge.hpp:40-70, robust_kernel_impl.cpp (Huber), types_six_dof_expmap.h:196-260 / .cpp:266-364, se3quat.h,
// linear_solver_dense.h:64-112 with Eigen's LDLT).  Double precision wherever g2o computes in double; float where the reference
// has float (the stereo edge's invz, the Huber dsqr member, deltaMono / deltaStereo, the chi2 of the classification).
//
// Work split: thread t of the 256 owns keypoints t, t + 256, ... (at most 32 of them: 8,192 keypoints).  Every
// pass over the edges -- errors + robust chi2 + the 6 x 6 normal equations, the chi2 of a trial, the classification -- sums the
// owning thread's edges in keypoint order and then combines the 256 partial sums in a fixed tree (wave butterfly, then the four
// waves in order): no atomics, and a problem's bits do not depend on the batch around it.  The 6 x 6 LDLT, the exp map and the
// quaternion products are computed by every lane from the same reduced values (identical bits in every lane: the result is
// wave-uniform without a broadcast barrier).  A keypoint's constants (observation, Xw, information, kind) are staged once in LDS
// for the first POSE_LDS_KP keypoints and read from the caller's arrays (L2) beyond that.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/orbslam_hip.h"
#include "common.h"
#include "orbm_g2o_math.h"
#include "orbm_internal.h"
#include "orbm_se3.h"

using namespace orbm_detail;

namespace {

constexpr int PT = 256;                 // threads per problem
constexpr int PW = PT / 64;             // waves
constexpr int POSE_MAXN = 8192;         // keypoints per problem (the resident-frame limit): 32 per thread, one bit each in a mask
constexpr int POSE_LDS_KP = 1024;       // keypoints whose constants are staged in LDS (32 B each)
constexpr int POSE_MAXLEVELS = 32;

struct PoseCam {
    double fx, fy, cx, cy, bf;
    float inv_sigma2[POSE_MAXLEVELS];
    int nlevels;
};

// the keypoint sources: host-array / device-array problems (orbx_keypoint by index) or a resident frame (SeqKp by sorted position)
struct PoseSrc {
    const orbx_keypoint *kps;   // [kp_off[B]] (array form) or nullptr
    const float *uright;        // [kp_off[B]] or nullptr (monocular)
    const SeqKp *fkp;           // resident frame: keypoints in sorted order
    const int *fperm;           //                 perm[sorted position] = keypoint index
    const uint8_t *has_mp;
    const float *mp_pos;
    const int *kp_off;          // [B + 1]
    const float *Tin;           // [B][16]
    // chained form (behind a projection search on the same stream): has_mp / mp_pos are not given, a keypoint's map point is formed
    // from the search's result -- the point match_kp[i] of the searched list, else the keypoint's base entry
    const int *match_kp;        // [n] by keypoint index: entry of the point list, < 0 none (device memory, written by the resolver)
    const float *pt_pos;        // [nq][3]
    const uint8_t *pt_takes;    // [nq]
    const uint8_t *base_has;    // [n] or nullptr: the slots the frame holds already (TrackLocalMap) ...
    const float *base_pos;      // [n][3]          ... their positions ...
    const uint8_t *base_takes;  // [n] or nullptr  ... and Observations() > 0 (nullptr: all)
    float4 *gathered;           // [n] scratch: (Xw, kind) of the keypoints behind the LDS-staged ones, formed once by the prologue
    const int *flags;           // the search's count and its generation-stamped "fixed point reached" word (SearchChain::Ctx)
    const int *overflow;        // the search's "a list outgrew its region" word
    int nq, gen, check_overflow, check_converged, min_matches;
};

struct PoseOut {
    float *Tout;                // [B][16]
    uint8_t *outlier;           // [kp_off[B]], written where has_mp
    int32_t *ngood;             // [B]
    orbm_pose_stats *stats;     // [B] or nullptr
    int32_t *track;             // chained form: status (TRACK_*), slots that are not outliers, those of them whose point is observed
};

enum { TRACK_SOLVED = 0, TRACK_SEARCH_AGAIN = 1, TRACK_FEW_MATCHES = 2, TRACK_REJECTED = 3 };

// ------------------------------------------------------------------ the edges

struct Edge { double obs[3], Xw[3], info; int kind; };   // kind 0: no map point, 1: mono, 2: stereo

// computeError of both pose-only edges (cam_project: .cpp:306-325)
__device__ __forceinline__ void edge_error(const PoseCam &c, const Edge &e, const Se3 &T, double err[3], double p[3])
{
    se3_map(T, e.Xw, p);
    if (e.kind == 1) {
        const double u = p[0] / p[2], v = p[1] / p[2];
        err[0] = e.obs[0] - (u * c.fx + c.cx);
        err[1] = e.obs[1] - (v * c.fy + c.cy);
        err[2] = 0.0;
    } else {
        const float invz = 1.0f / p[2];
        const double r0 = p[0] * invz * c.fx + c.cx;
        const double r1 = p[1] * invz * c.fy + c.cy;
        const double r2 = r0 - c.bf * invz;
        err[0] = e.obs[0] - r0; err[1] = e.obs[1] - r1; err[2] = e.obs[2] - r2;
    }
}

// BaseEdge::chi2 with a diagonal information matrix (the off-diagonal zeros multiplied, as in the restatement)
__device__ __forceinline__ double edge_chi2(const Edge &e, const double err[3])
{
    const int D = e.kind == 2 ? 3 : 2;
    double oe[3];
    ORBM_UNROLL for (int i = 0; i < 3; ++i) {
        double s = ((i == 0) ? e.info : 0.0) * err[0];
        ORBM_UNROLL for (int j = 1; j < 3; ++j) if (j < D) s += ((i == j) ? e.info : 0.0) * err[j];
        oe[i] = s;
    }
    double r = err[0] * oe[0];
    ORBM_UNROLL for (int i = 1; i < 3; ++i) if (i < D) r += err[i] * oe[i];
    return r;
}

// linearizeOplus of both edges at the mapped point p
__device__ __forceinline__ void edge_jacobian(const PoseCam &c, int kind, const double p[3], double J[18])
{
    const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
    J[0] = x * y * invz_2 * c.fx; J[1] = -(1 + (x * x * invz_2)) * c.fx; J[2] = y * invz * c.fx;
    J[3] = -invz * c.fx;          J[4] = 0;                               J[5] = x * invz_2 * c.fx;
    J[6] = (1 + y * y * invz_2) * c.fy; J[7] = -x * y * invz_2 * c.fy; J[8] = -x * invz * c.fy;
    J[9] = 0;                           J[10] = -invz * c.fy;          J[11] = y * invz_2 * c.fy;
    if (kind == 2) {
        J[12] = J[0] - c.bf * y * invz_2; J[13] = J[1] + c.bf * x * invz_2; J[14] = J[2];
        J[15] = J[3];                     J[16] = 0;                        J[17] = J[5] - c.bf * invz_2;
    }
}

constexpr int NSYS = 21 + 6 + 1;    // lower triangle of H, A^T w omega e, robust chi2 (the block sums: orbm_g2o_math.h)

// SRC 0: keypoints from arrays, 1: from a resident frame, 2: resident frame + the map points of a search's result (chained)
template <int SRC>
__global__ __launch_bounds__(PT) void k_pose_optimization(PoseSrc src, PoseCam cam, PoseOut out)
{
    constexpr bool FRAME = SRC >= 1, CHAIN = SRC == 2;
    __shared__ float4 s_a[POSE_LDS_KP], s_b[POSE_LDS_KP];   // (obs x, obs y, ur, info), (Xw, kind)
    __shared__ uint16_t s_inv[FRAME ? POSE_MAXN : 1];        // resident frame: sorted position of keypoint i
    __shared__ double s_red[PW][NSYS];
    __shared__ int s_ired[PW];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int base = src.kp_off[b], n = src.kp_off[b + 1] - base;
    const float *Tin = src.Tin + 16 * b;
    if (n < 0 || n > POSE_MAXN) {
        if (tid == 0) { out.ngood[b] = ORBX_ERR_UNSUPPORTED; if (CHAIN) out.track[0] = TRACK_REJECTED; }
        return;
    }
    if (CHAIN) {
        // the search in front may have to be repeated (a window list outgrew its region, the resolver's fixed point was not reached)
        // or found too few matches: the host sees the same words after its wait; nothing is solved on such a result
        const bool again = (src.check_overflow && *src.overflow == src.gen) || (src.check_converged && src.flags[2] != src.gen);
        if (again || src.flags[0] < src.min_matches) {
            if (tid == 0) out.track[0] = again ? TRACK_SEARCH_AGAIN : TRACK_FEW_MATCHES;
            return;
        }
    }
    // mvpMapPoints[i] != NULL; chained: the entry of the searched list (>= 0), the base entry (-1) or none (-2)
    auto slot = [&](int i) -> int {
        const int q = src.match_kp[i];
        if (q >= 0 && q < src.nq) return q;
        return (src.base_has && src.base_has[i]) ? -1 : -2;
    };
    auto has_at = [&](int i) -> bool { return CHAIN ? slot(i) > -2 : src.has_mp[base + i] != 0; };
    if (FRAME) {
        for (int sp = tid; sp < n; sp += PT) s_inv[src.fperm[sp]] = (uint16_t)sp;
        __syncthreads();
    }

    // one keypoint's edge constants, from the caller's arrays (Optimizer.cc:303-383)
    bool staged = false;
    auto fetch = [&](int i, float4 &a, float4 &c) {
        const int g = base + i;
        float kx, ky, ur; int oct;
        if (FRAME) {
            const SeqKp k = src.fkp[s_inv[i]];
            kx = k.x; ky = k.y; ur = k.uright; oct = k.octave;
        } else {
            const orbx_keypoint &k = src.kps[g];
            kx = k.x; ky = k.y; oct = k.octave;
            ur = src.uright ? src.uright[g] : -1.0f;
        }
        oct = oct < 0 ? 0 : (oct >= POSE_MAXLEVELS ? POSE_MAXLEVELS - 1 : oct);
        a = make_float4(kx, ky, ur, cam.inv_sigma2[oct]);
        if (CHAIN && staged && i >= POSE_LDS_KP) { c = src.gathered[i]; return; }     // (its own thread wrote it: no barrier needed)
        const float *P = nullptr;
        if (CHAIN) {
            const int q = slot(i);
            if (q > -2) P = q >= 0 ? src.pt_pos + 3 * (size_t)q : src.base_pos + 3 * (size_t)i;
        } else if (src.has_mp[g]) P = src.mp_pos + 3 * (size_t)g;
        c = P ? make_float4(P[0], P[1], P[2], ur < 0 ? 1.f : 2.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    int nloc = 0;
    for (int i = tid; i < n && i < POSE_LDS_KP; i += PT, ++nloc) fetch(i, s_a[i], s_b[i]);
    if (CHAIN) {        // the gather runs once, here: the passes read one float4 per keypoint behind the LDS-staged ones
        for (int i = POSE_LDS_KP + tid; i < n; i += PT) {
            float4 a, c;
            fetch(i, a, c);
            src.gathered[i] = c;
        }
        staged = true;
    }
    auto edge = [&](int i, Edge &e) {
        float4 a, c;
        if (i < POSE_LDS_KP) { a = s_a[i]; c = s_b[i]; }
        else fetch(i, a, c);
        e.obs[0] = a.x; e.obs[1] = a.y; e.obs[2] = a.z; e.info = a.w;
        e.Xw[0] = c.x; e.Xw[1] = c.y; e.Xw[2] = c.z; e.kind = (int)c.w;
    };
    (void)nloc;

    // nInitialCorrespondences (every keypoint with a map point gives one edge; mvbOutlier = false).  A map point on a keypoint
    // whose octave has no mvInvLevelSigma2 entry (the host forms refuse it before the launch) rejects the problem: ORBX_ERR_ARG
    // and no other output.  Counted as 1 << 16 each: both sums fit in one reduction (at most 8,192 keypoints).
    int mine = 0;
    for (int i = tid; i < n; i += PT) {
        if (!has_at(i)) continue;
        const int oct = FRAME ? src.fkp[s_inv[i]].octave : src.kps[base + i].octave;
        mine += (oct < 0 || oct >= cam.nlevels) ? (1 << 16) : 1;
    }
    const int counts = block_sum_int<PW>(mine, s_ired);
    if (counts >> 16) {
        if (tid == 0) { out.ngood[b] = ORBX_ERR_ARG; if (CHAIN) out.track[0] = TRACK_REJECTED; }
        return;
    }
    const int nInitial = counts;

    const float deltaMono = sqrt(5.991), deltaStereo = sqrt(7.815);
    const float chi2Mono = 5.991f, chi2Stereo = 7.815f;

    uint32_t lvl = 0;                       // bit k: the k-th owned keypoint's edge is at level 1 (mvbOutlier)
    // chained: the loops behind the solve (Tracking.cc:1257-1276, :1301-1320) -- slots that are not outliers, and those of them
    // whose point has Observations() > 0 -- as one block sum (16 bits each: at most 8,192 keypoints)
    auto tally = [&]() {
        int mine = 0, k = 0;
        for (int i = tid; i < n; i += PT, ++k) {
            const int q = slot(i);
            if (q == -2 || ((lvl >> k) & 1u)) continue;
            const bool takes = q >= 0 ? src.pt_takes[q] != 0 : (!src.base_takes || src.base_takes[i] != 0);
            mine += 1 + (takes ? (1 << 16) : 0);
        }
        const int c = block_sum_int<PW>(mine, s_ired);
        if (tid == 0) { out.track[0] = TRACK_SOLVED; out.track[1] = c & 0xffff; out.track[2] = c >> 16; }
    };

    orbm_pose_stats st;
    memset(&st, 0, sizeof(st));
    st.ninitial = nInitial;
    if (nInitial < 3) {
        for (int i = tid; i < n; i += PT)
            if (has_at(i)) out.outlier[base + i] = 0;
        if (CHAIN) tally();
        if (tid < 16) out.Tout[16 * b + tid] = Tin[tid];
        if (tid == 0) {
            out.ngood[b] = 0;
            if (out.stats) out.stats[b] = st;
        }
        return;
    }

    Se3 est, eval;                          // the estimate; the pose of the last computeActiveErrors
    int nBad = 0;
    for (int it = 0; it < 4; ++it) {
        const bool robust = it < 3;         // setRobustKernel(0) after the classification of it == 2
        se3_from_cv(Tin, est);
        const int nactive = nInitial - nBad;
        int iters = 0, trials = 0;
        double currentChiOut = 0.0;

        // one pass: errors at T, robust chi2 and (with SYS) the normal equations; returns the block totals in v
        auto pass = [&](const Se3 &T, bool sys, double (&v)[NSYS]) {
            for (int j = 0; j < NSYS; ++j) v[j] = 0.0;
            int k = 0;
            for (int i = tid; i < n; i += PT, ++k) {
                if ((lvl >> k) & 1u) continue;
                Edge e;
                edge(i, e);
                if (!e.kind) continue;
                double err[3], p[3];
                edge_error(cam, e, T, err, p);
                const double chi2 = edge_chi2(e, err);
                double rho0 = chi2, w = 1.0;
                if (robust) huber(chi2, e.kind == 2 ? (double)deltaStereo : (double)deltaMono, rho0, w);
                v[27] += rho0;
                if (!sys) continue;
                double J[18];
                edge_jacobian(cam, e.kind, p, J);
                const int D = e.kind == 2 ? 3 : 2;
                const double winfo = w * e.info;
                ORBM_UNROLL for (int r = 0; r < 6; ++r) {
                    double s = 0;
                    ORBM_UNROLL for (int ii = 0; ii < 3; ++ii) if (ii < D) s += J[6 * ii + r] * (e.info * err[ii]);
                    v[21 + r] += w * s;
                    ORBM_UNROLL for (int c = 0; c <= r; ++c) {
                        double hh = 0;
                        ORBM_UNROLL for (int ii = 0; ii < 3; ++ii) if (ii < D) hh += J[6 * ii + r] * (winfo * J[6 * ii + c]);
                        v[r * (r + 1) / 2 + c] += hh;
                    }
                }
            }
            if (sys) block_sum<NSYS, PW>(v, s_red);
            else {
                double c1[1] = {v[27]};
                block_sum<1, PW>(c1, s_red);
                v[27] = c1[0];
            }
        };

        if (nactive > 0) {
            LmStep lm;
            for (int iteration = 0; iteration < 10; ++iteration) {      // SparseOptimizer::optimize
                ++iters;
                double v[NSYS];
                pass(est, true, v);                                     // computeActiveErrors, activeRobustChi2, buildSystem
                eval = est;
                double currentChi = v[27];
                const double iniChi = currentChi;
                double H[36], bb[6];
                for (int r = 0, h = 0; r < 6; ++r)
                    for (int c = 0; c <= r; ++c, ++h) H[6 * r + c] = v[h];
                for (int r = 0; r < 6; ++r) bb[r] = -v[21 + r];
                if (iteration == 0) {                                   // computeLambdaInit, tau = 1e-5
                    double maxDiagonal = 0.;
                    for (int j = 0; j < 6; ++j) { const double f = fabs(H[7 * j]); maxDiagonal = (f < maxDiagonal) ? maxDiagonal : f; }
                    lm.start(1e-5 * maxDiagonal);
                }
                double rho = 0;
                int qmax = 0;
                do {
                    double Hl[36], x[6] = {0, 0, 0, 0, 0, 0};
                    for (int j = 0; j < 36; ++j) Hl[j] = H[j];
                    for (int j = 0; j < 6; ++j) Hl[7 * j] += lm.lambda;
                    const bool ok2 = ldlt_solve<6, LdltZeroDiagonal::ReturnZero>(Hl, bb, x);
                    Se3 up, trial;
                    se3_exp(x, up);
                    se3_compose(up, est, trial);
                    double cv[NSYS];
                    pass(trial, false, cv);
                    eval = trial;
                    double tempChi = cv[27];
                    if (!ok2) tempChi = 1.7976931348623157e308;
                    double scale = 0.;
                    for (int j = 0; j < 6; ++j) scale += x[j] * (lm.lambda * x[j] + bb[j]);
                    rho = lm.verdict(currentChi, tempChi, scale, [&]() { est = trial; }).rho;
                    qmax++;
                } while (rho < 0 && qmax < 10);
                trials += qmax;
                currentChiOut = currentChi;
                if (lm.end_iteration(qmax, rho, iniChi, currentChi) != 1) break;
            }
        }
        st.rounds = it + 1; st.iterations[it] = iters; st.trials[it] = trials; st.chi2 = currentChiOut;

        // classification (Optimizer.cc:393-448): level-1 edges recompute their error at the estimate, active edges keep the
        // error of the last computeActiveErrors (at `eval`, the last TRIED pose)
        int bad = 0, k = 0;
        for (int i = tid; i < n; i += PT, ++k) {
            Edge e;
            edge(i, e);
            if (!e.kind) continue;
            const bool was_out = (lvl >> k) & 1u;
            double err[3], p[3];
            edge_error(cam, e, was_out ? est : eval, err, p);
            const float chi2 = edge_chi2(e, err);
            if (chi2 > (e.kind == 2 ? chi2Stereo : chi2Mono)) { lvl |= 1u << k; bad++; }
            else lvl &= ~(1u << k);
        }
        nBad = block_sum_int<PW>(bad, s_ired);
        if (nInitial < 10) break;                                       // optimizer.edges().size() < 10
    }

    int k = 0;
    for (int i = tid; i < n; i += PT, ++k)
        if (has_at(i)) out.outlier[base + i] = (lvl >> k) & 1u;
    if (CHAIN) tally();
    if (tid == 0) {
        double R[9];
        quat_to_matrix(est.q, R);                                       // Converter::toCvMat(SE3Quat)
        float *T = out.Tout + 16 * b;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
            T[4 * i + 3] = (float)est.t[i];
        }
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        out.ngood[b] = nInitial - nBad;
        if (out.stats) {
            for (int j = 0; j < 4; ++j) st.q[j] = est.q[j];
            for (int j = 0; j < 3; ++j) st.t[j] = est.t[j];
            out.stats[b] = st;
        }
    }
}

int make_cam(const orbm_pose_camera *c, PoseCam &pc)
{
    if (!c || c->nlevels < 1 || c->nlevels > POSE_MAXLEVELS || !c->inv_level_sigma2) return -1;
    memset(&pc, 0, sizeof(pc));
    pc.fx = c->fx; pc.fy = c->fy; pc.cx = c->cx; pc.cy = c->cy; pc.bf = c->bf;
    for (int l = 0; l < c->nlevels; ++l) pc.inv_sigma2[l] = c->inv_level_sigma2[l];
    pc.nlevels = c->nlevels;
    return 0;
}

int check_octaves_host(const orbx_keypoint *kps, const uint8_t *has_mp, int n, int nlevels)
{
    for (int i = 0; i < n; ++i)
        if (has_mp[i] && (kps[i].octave < 0 || kps[i].octave >= nlevels)) return -1;
    return 0;
}

// the host-array forms: stage everything, one launch, one download, scatter the outlier flags where has_mp
int pose_host(const orbx_keypoint *kps, const float *uright, const int32_t *kp_off, int batch, const uint8_t *has_mp, const float *mp_pos,
              const PoseCam &pc, const float *Tin, float *Tout, uint8_t *outlier, int32_t *ngood, orbm_pose_stats *stats)
{
    const int total = kp_off[batch];
    StagedCall sc;
    const size_t o_k = sc.in(kps, sizeof(orbx_keypoint) * (size_t)total), o_u = uright ? sc.in(uright, sizeof(float) * (size_t)total) : 0,
                 o_h = sc.in(has_mp, (size_t)total), o_p = sc.in(mp_pos, sizeof(float) * 3 * (size_t)total),
                 o_o = sc.in(kp_off, sizeof(int32_t) * (size_t)(batch + 1)), o_t = sc.in(Tin, sizeof(float) * 16 * (size_t)batch);
    const size_t r_t = sc.out(sizeof(float) * 16 * (size_t)batch), r_g = sc.out(sizeof(int32_t) * (size_t)batch),
                 r_s = sc.out(sizeof(orbm_pose_stats) * (size_t)batch), r_o = sc.out((size_t)total);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    PoseSrc src = {sc.d<orbx_keypoint>(o_k), uright ? sc.d<float>(o_u) : nullptr, nullptr, nullptr, sc.d<uint8_t>(o_h), sc.d<float>(o_p),
                   sc.d<int>(o_o), sc.d<float>(o_t)};
    PoseOut po = {sc.d<float>(r_t), sc.d<uint8_t>(r_o), sc.d<int32_t>(r_g), sc.d<orbm_pose_stats>(r_s)};
    hipLaunchKernelGGL(k_pose_optimization<0>, dim3(batch), dim3(PT), 0, sc.stream(), src, pc, po);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(Tout, sc.r<float>(r_t), sizeof(float) * 16 * (size_t)batch);
    memcpy(ngood, sc.r<int32_t>(r_g), sizeof(int32_t) * (size_t)batch);
    if (stats) memcpy(stats, sc.r<orbm_pose_stats>(r_s), sizeof(orbm_pose_stats) * (size_t)batch);
    const uint8_t *o = sc.r<uint8_t>(r_o);
    for (int i = 0; i < total; ++i)
        if (has_mp[i]) outlier[i] = o[i];
    for (int p = 0; p < batch; ++p)
        if (ngood[p] < 0) ORBX_FAIL(ngood[p], "pose problem rejected by the kernel");
    return ORBX_OK;
}

std::atomic<int> g_last_track_waits{0};    // host waits of the last tracking call of this process

// The pose solve as the tail of a projection search (SearchChain): its inputs travel with the search's upload, the kernel is
// enqueued behind the resolver and forms its edges from the resolver's match_kp in device memory, and its results are written
// into the pinned result block behind the search's.
struct PoseChain : SearchChain {
    // set by the caller
    const orbm_frame *fr = nullptr;
    PoseCam pc;
    const float *Tcw = nullptr;
    const orbm_points *pts = nullptr;
    const uint8_t *base_has = nullptr, *base_takes = nullptr;
    const float *base_pos = nullptr;
    int min_matches = 0;
    const int32_t *match_kp = nullptr;      // the search's host result (filled when collect() runs)
    float *Tcw_out = nullptr;
    uint8_t *outlier = nullptr;
    orbm_pose_stats *stats = nullptr;
    // results
    int status = -1, ngood = 0, nmatches = 0, nmatches_map = 0;

    size_t o_t = 0, o_off = 0, o_pp = 0, o_bh = 0, o_bp = 0, o_bt = 0, r_t = 0, r_g = 0, r_s = 0, r_k = 0, r_o = 0, x_g = 0;
    void carve_inputs(Workspace &w) override
    {
        const size_t n = fr->n ? (size_t)fr->n : 1, m = pts->n ? (size_t)pts->n : 1;
        o_t = w.carve(sizeof(float) * 16); o_off = w.carve(2 * sizeof(int32_t)); o_pp = w.carve(sizeof(float) * 3 * m);
        o_bh = w.carve(base_has ? n : 1); o_bp = w.carve(base_has ? sizeof(float) * 3 * n : 1); o_bt = w.carve(base_has && base_takes ? n : 1);
    }
    void fill_inputs(Workspace &w) override
    {
        const int32_t off[2] = {0, fr->n};
        memcpy(w.h<char>(o_t), Tcw, sizeof(float) * 16);
        memcpy(w.h<char>(o_off), off, sizeof(off));
        if (pts->n) memcpy(w.h<char>(o_pp), pts->pos, sizeof(float) * 3 * (size_t)pts->n);
        if (base_has && fr->n) {
            memcpy(w.h<char>(o_bh), base_has, (size_t)fr->n);
            memcpy(w.h<char>(o_bp), base_pos, sizeof(float) * 3 * (size_t)fr->n);
            if (base_takes) memcpy(w.h<char>(o_bt), base_takes, (size_t)fr->n);
        }
    }
    void carve_results(Workspace &w) override
    {
        r_t = w.carve(sizeof(float) * 16); r_g = w.carve(sizeof(int32_t)); r_s = w.carve(sizeof(orbm_pose_stats));
        r_k = w.carve(4 * sizeof(int32_t)); r_o = w.carve(fr->n ? (size_t)fr->n : 1);
        x_g = w.carve(sizeof(float4) * (size_t)(fr->n ? fr->n : 1));      // device scratch (behind the results: never read back)
    }
    template <typename T> static T *res(const Ctx &c, size_t off) { return reinterpret_cast<T *>(c.w->pin + (off - c.o_res)); }
    int launch(const Ctx &c) override
    {
        const Workspace &w = *c.w;
        PoseSrc src = {nullptr, nullptr, fr->kp, fr->perm, nullptr, nullptr, w.d<int>(o_off), w.d<float>(o_t),
                       c.match_kp, w.d<float>(o_pp), c.qtakes, base_has ? w.d<uint8_t>(o_bh) : nullptr, w.d<float>(o_bp),
                       base_has && base_takes ? w.d<uint8_t>(o_bt) : nullptr, w.d<float4>(x_g), c.flags, c.overflow, c.nq, c.gen, c.check_overflow ? 1 : 0,
                       c.check_converged ? 1 : 0, min_matches};
        // (the results go straight into the pinned block, as the parallel resolver's do: posted writes, no copy behind the kernel)
        PoseOut po = {res<float>(c, r_t), res<uint8_t>(c, r_o), res<int32_t>(c, r_g), res<orbm_pose_stats>(c, r_s), res<int32_t>(c, r_k)};
        hipLaunchKernelGGL(k_pose_optimization<2>, dim3(1), dim3(PT), 0, c.st, src, pc, po);
        ORBX_HIP(hipGetLastError());
        return ORBX_OK;
    }
    void collect(const Ctx &c) override
    {
        const int32_t *k = res<int32_t>(c, r_k);
        status = k[0];
        if (status != TRACK_SOLVED) return;
        nmatches = k[1]; nmatches_map = k[2];
        ngood = *res<int32_t>(c, r_g);
        memcpy(Tcw_out, res<float>(c, r_t), sizeof(float) * 16);
        if (stats) memcpy(stats, res<orbm_pose_stats>(c, r_s), sizeof(orbm_pose_stats));
        const uint8_t *o = res<uint8_t>(c, r_o);
        for (int j = 0; j < fr->n; ++j)
            if (match_kp[j] >= 0 || (base_has && base_has[j])) outlier[j] = o[j];
    }
};

// what both tracking calls check before anything is launched
int track_prepare(const orbm_frame *cur, const orbm_view *view, const orbm_pose_camera *cam, PoseChain &ch)
{
    if (make_cam(cam, ch.pc)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ch.fr = cur;
    if (ch.fr->n > POSE_MAXN) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in one pose problem");
    if (ch.fr->min_octave < 0 || ch.fr->max_octave >= cam->nlevels || ch.fr->max_octave >= view->nlevels)
        ORBX_FAIL(ORBX_ERR_ARG, "keypoint octave outside the view's or the pose camera's levels");
    return ORBX_OK;
}

} // namespace

int orbm_pose_optimization(const orbx_keypoint *kps_un, const float *uright, int n, const uint8_t *has_mp, const float *mp_pos,
                           const orbm_pose_camera *cam, const float *Tcw_in, float *Tcw_out, uint8_t *outlier, int *ngood,
                           orbm_pose_stats *stats)
{
    PoseCam pc;
    if (n < 0 || (n && (!kps_un || !has_mp || !mp_pos || !outlier)) || !Tcw_in || !Tcw_out || !ngood || make_cam(cam, pc))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > POSE_MAXN) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in one pose problem");
    if (check_octaves_host(kps_un, has_mp, n, cam->nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "keypoint octave outside mvInvLevelSigma2");
    ORBX_NEED_DEVICE();
    const int32_t off[2] = {0, n};
    return pose_host(kps_un, uright, off, 1, has_mp, mp_pos, pc, Tcw_in, Tcw_out, outlier, ngood, stats);
}

int orbm_frame_pose_optimization(const orbm_frame *frame, const uint8_t *has_mp, const float *mp_pos, const orbm_pose_camera *cam,
                                 const float *Tcw_in, float *Tcw_out, uint8_t *outlier, int *ngood, orbm_pose_stats *stats)
{
    PoseCam pc;
    if (!frame || !Tcw_in || !Tcw_out || !ngood || make_cam(cam, pc)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    const int n = frame->n;
    if (n && (!has_mp || !mp_pos || !outlier)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > POSE_MAXN) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in one pose problem");
    if (frame->min_octave < 0 || frame->max_octave >= cam->nlevels) ORBX_FAIL(ORBX_ERR_ARG, "keypoint octave outside mvInvLevelSigma2");
    const int32_t off[2] = {0, n};
    StagedCall sc;
    const size_t o_h = sc.in(has_mp, (size_t)n), o_p = sc.in(mp_pos, sizeof(float) * 3 * (size_t)n), o_o = sc.in(off, sizeof(off)),
                 o_t = sc.in(Tcw_in, sizeof(float) * 16);
    const size_t r_t = sc.out(sizeof(float) * 16), r_g = sc.out(sizeof(int32_t)), r_s = sc.out(sizeof(orbm_pose_stats)), r_o = sc.out((size_t)n);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    PoseSrc src = {nullptr, nullptr, frame->kp, frame->perm, sc.d<uint8_t>(o_h), sc.d<float>(o_p), sc.d<int>(o_o), sc.d<float>(o_t)};
    PoseOut po = {sc.d<float>(r_t), sc.d<uint8_t>(r_o), sc.d<int32_t>(r_g), sc.d<orbm_pose_stats>(r_s)};
    hipLaunchKernelGGL(k_pose_optimization<1>, dim3(1), dim3(PT), 0, sc.stream(), src, pc, po);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(Tcw_out, sc.r<float>(r_t), sizeof(float) * 16);
    *ngood = *sc.r<int32_t>(r_g);
    if (stats) memcpy(stats, sc.r<orbm_pose_stats>(r_s), sizeof(orbm_pose_stats));
    const uint8_t *o = sc.r<uint8_t>(r_o);
    for (int i = 0; i < n; ++i)
        if (has_mp[i]) outlier[i] = o[i];
    return ORBX_OK;
}

int orbm_pose_optimization_batch(const orbx_keypoint *kps_un, const float *uright, const int32_t *kp_off, int batch, const uint8_t *has_mp,
                                 const float *mp_pos, const orbm_pose_camera *cam, const float *Tcw_in, float *Tcw_out, uint8_t *outlier,
                                 int32_t *ngood, orbm_pose_stats *stats, int is_device, void *stream)
{
    PoseCam pc;
    if (batch < 0 || !kp_off || !Tcw_in || !Tcw_out || !ngood || make_cam(cam, pc)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (batch == 0) return ORBX_OK;
    if (is_device) {
        if (!kps_un || !has_mp || !mp_pos || !outlier) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        ORBX_NEED_DEVICE();
        PoseSrc src = {kps_un, uright, nullptr, nullptr, has_mp, mp_pos, kp_off, Tcw_in};
        PoseOut po = {Tcw_out, outlier, ngood, stats};
        hipLaunchKernelGGL(k_pose_optimization<0>, dim3(batch), dim3(PT), 0, (hipStream_t)stream, src, pc, po);
        ORBX_HIP(hipGetLastError());
        return ORBX_OK;
    }
    if (kp_off[0] != 0) ORBX_FAIL(ORBX_ERR_ARG, "kp_off[0] must be 0");
    for (int p = 0; p < batch; ++p) {
        const int np = kp_off[p + 1] - kp_off[p];
        if (np < 0) ORBX_FAIL(ORBX_ERR_ARG, "kp_off must not decrease");
        if (np > POSE_MAXN) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 keypoints in one pose problem");
    }
    const int total = kp_off[batch];
    if (total && (!kps_un || !has_mp || !mp_pos || !outlier)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (check_octaves_host(kps_un, has_mp, total, cam->nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "keypoint octave outside mvInvLevelSigma2");
    ORBX_NEED_DEVICE();
    return pose_host(kps_un, uright, kp_off, batch, has_mp, mp_pos, pc, Tcw_in, Tcw_out, outlier, ngood, stats);
}

int orbm_debug_last_track_waits(void) { return g_last_track_waits.load(std::memory_order_relaxed); }

int orbm_track_with_motion_model(const orbm_frame *cur, const orbm_view *view, const orbm_pose_camera *cam, const float *Tcw, const float *Tlw,
                                 const orbm_points *last, float th, int mono, int th_high, int check_orientation, int min_matches,
                                 int32_t *match_kp, int32_t *match_q, uint8_t *outlier, float *Tcw_out, orbm_track_result *result,
                                 orbm_pose_stats *stats)
{
    if (!cur || !view || !cam || !Tcw || !Tlw || !last || !Tcw_out || !result) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    PoseChain ch;
    const int rc0 = track_prepare(cur, view, cam, ch);
    if (rc0 != ORBX_OK) return rc0;
    if (ch.fr->n && (!match_kp || !outlier)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    memset(result, 0, sizeof(*result));
    memcpy(Tcw_out, Tcw, sizeof(float) * 16);
    if (stats) memset(stats, 0, sizeof(*stats));
    ch.Tcw = Tcw; ch.pts = last; ch.min_matches = min_matches; ch.match_kp = match_kp; ch.Tcw_out = Tcw_out; ch.outlier = outlier;
    ch.stats = stats;
    int nm = 0;
    for (int pass = 1; pass <= 2; ++pass) {     // Tracking.cc:1242-1249: th, then 2 * th from scratch
        ch.status = -1;
        const int rc = search_by_projection_last_chain(cur, view, Tcw, Tlw, last, nullptr, pass == 1 ? th : 2 * th, mono, th_high,
                                                       check_orientation, match_kp, match_q, &nm, nullptr, &ch);
        g_last_track_waits.store(ch.waits, std::memory_order_relaxed);
        if (rc != ORBX_OK) return rc;
        result->search_used = pass; result->nsearch = nm;
        if (nm >= min_matches) break;
    }
    if (nm < min_matches) return ORBX_OK;       // :1251-1252
    result->tracked = 1;
    if (!ch.launched) return ORBX_OK;           // nothing was searched (no point, no keypoint in the grid): no edge, the pose stands
    if (ch.status != TRACK_SOLVED) ORBX_FAIL(ch.status == TRACK_REJECTED ? ORBX_ERR_ARG : ORBX_ERR_HIP, "the chained pose solve did not run");
    result->ngood = ch.ngood; result->nmatches = ch.nmatches; result->nmatches_map = ch.nmatches_map;
    return ORBX_OK;
}

int orbm_track_local_map(const orbm_frame *cur, const orbm_view *view, const orbm_pose_camera *cam, const float *Tcw, const orbm_points *points,
                         const uint8_t *base_has, const float *base_pos, const uint8_t *base_takes, float th, float viewing_cos_limit,
                         int th_high, float nnratio, int32_t *match_kp, int32_t *match_q, orbm_projected_point *projected_out,
                         uint8_t *outlier, float *Tcw_out, orbm_track_result *result, orbm_pose_stats *stats)
{
    if (!cur || !view || !cam || !Tcw || !points || !Tcw_out || !result || (base_has && !base_pos)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    PoseChain ch;
    const int rc0 = track_prepare(cur, view, cam, ch);
    if (rc0 != ORBX_OK) return rc0;
    const int n = ch.fr->n;
    if (n && (!match_kp || !outlier)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    memset(result, 0, sizeof(*result));
    memcpy(Tcw_out, Tcw, sizeof(float) * 16);
    if (stats) memset(stats, 0, sizeof(*stats));
    std::vector<uint8_t> occ((size_t)(n ? n : 1), 0);       // ORBmatcher.cc:87-89: the slot holds an observed point
    for (int j = 0; j < n && base_has; ++j) occ[j] = base_has[j] && (!base_takes || base_takes[j]);
    ch.Tcw = Tcw; ch.pts = points; ch.min_matches = INT32_MIN; ch.match_kp = match_kp; ch.Tcw_out = Tcw_out; ch.outlier = outlier;
    ch.stats = stats; ch.base_has = base_has; ch.base_pos = base_pos; ch.base_takes = base_takes;
    int nm = 0;
    const int rc = search_by_projection_points_chain(cur, view, Tcw, points, base_has ? occ.data() : nullptr, th, viewing_cos_limit, th_high,
                                                     nnratio, match_kp, match_q, &nm, projected_out, nullptr, &ch);
    g_last_track_waits.store(ch.waits, std::memory_order_relaxed);
    if (rc != ORBX_OK) return rc;
    result->search_used = 1; result->nsearch = nm; result->tracked = 1;
    if (ch.launched) {
        if (ch.status != TRACK_SOLVED) ORBX_FAIL(ch.status == TRACK_REJECTED ? ORBX_ERR_ARG : ORBX_ERR_HIP, "the chained pose solve did not run");
        result->ngood = ch.ngood; result->nmatches = ch.nmatches; result->nmatches_map = ch.nmatches_map;
        return ORBX_OK;
    }
    // nothing was searched (an empty point list, no keypoint inside the grid): the solve over the slots the frame holds already
    if (!n || !base_has) return ORBX_OK;
    int ngood = 0;
    const int rcp = orbm_frame_pose_optimization(cur, base_has, base_pos, cam, Tcw, Tcw_out, outlier, &ngood, stats);
    g_last_track_waits.store(ch.waits + 1, std::memory_order_relaxed);
    if (rcp != ORBX_OK) return rcp;
    result->ngood = ngood;
    for (int j = 0; j < n; ++j)
        if (base_has[j] && !outlier[j]) { result->nmatches++; result->nmatches_map += !base_takes || base_takes[j]; }
    return ORBX_OK;
}
