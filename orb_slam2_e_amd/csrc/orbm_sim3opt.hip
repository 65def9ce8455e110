// orbm_sim3opt.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1425-1625) from :1564 on as ONE launch: one workgroup per loop candidate
// runs optimize(5), the outlier cut, optimize(5 or 10) and the final count, on g2o's code paths (Thirdparty/g2o/g2o: types/sim3.h,
// types/types_seven_dof_expmap.h:60-69 / :138-167, core/base_binary_edge.hpp:55-120 and the numeric linearizeOplus :131-205,
// core/optimization_algorithm_levenberg.cpp:63-268, core/sparse_optimizer.cpp:425-504, robust_kernel_impl.cpp (Huber),
// solvers/linear_solver_dense.h:64-112 with Eigen's LDLT).  Double precision wherever g2o computes in double; float where the
// reference has float (R * Xw + t of the cv::Mat points, deltaHuber, the Huber dsqr member, th2).
//
// Work split: thread t of the 256 owns pairs t, t + 256, ...  An iteration's 14 perturbed estimates
// Sim3(+-1e-9 e_d) * estimate and their inverses are the same for every edge: lanes 0 .. 13 compute one each into LDS, once per
// iteration.  Every pass over the pairs -- errors + numeric Jacobians + robust chi2 + the 7 x 7 normal equations, the chi2 of a
// trial, the cut -- sums the owning thread's pairs in index order (e12, then e21) and then combines the partial sums in a fixed
// tree (wave butterfly, then the waves in order): no atomics, and a problem's bits do not depend on the batch around it.  The
// 7 x 7 LDLT, Sim3(update), the compose and the inverse are computed by every lane from the same reduced values (identical bits in
// every lane: wave-uniform without a broadcast barrier).  A pair's constants are staged once, in LDS for the first SO_LDS_PAIRS
// pairs and in the workspace beyond.  The quaternion / LDLT / Huber helpers and the reductions are the ones orbm_pose.hip uses
// (orbm_g2o_math.h); g2o's Sim3 with its exp, product and inverse is orbm_sim3_math.h, which orbm_essential_graph.hip shares.
#include <atomic>

#include "orbm_g2o_math.h"
#include "orbm_internal.h"
#include "orbm_sim3_math.h"
#include "orbm_sim3opt_internal.h"

using namespace orbm_detail;

namespace {

constexpr int SO_NT = 256;              // threads per problem: four waves (one wave, NT = 64, was measured too and lost: DESIGN.md 14)
constexpr int SO_NSYS = 28 + 7 + 1;     // lower triangle of H, J^T rho1 omega e, robust chi2

struct PairC { float v[12]; };          // Xc1 [3], Xc2 [3], obs1 [2], obs2 [2], info1, info2
static_assert(sizeof(PairC) == SO_PAIR_BYTES, "the o_pair scratch is sized by SO_PAIR_BYTES");

// computeError of EdgeSim3ProjectXYZ (S = the estimate, X = the point of keyframe 2) and of EdgeInverseSim3ProjectXYZ (S = its
// inverse, X = the point of keyframe 1): obs - cam_map(project(S.map(X)))
__device__ __forceinline__ void edge_error(const Sim3 &S, const double X[3], const double obs[2], const float *cam, double e[2])
{
    double p[3];
    q_rotate(S.q, X, p);
    ORBM_UNROLL for (int k = 0; k < 3; ++k) p[k] = S.s * p[k] + S.t[k];
    const double u = p[0] / p[2], v = p[1] / p[2];
    e[0] = obs[0] - (u * (double)cam[0] + (double)cam[2]);
    e[1] = obs[1] - (v * (double)cam[1] + (double)cam[3]);
}

__device__ __forceinline__ double edge_chi2(double info, const double e[2])   // _error.dot(information() * _error), information = info * I
{
    const double o0 = info * e[0] + 0.0 * e[1], o1 = 0.0 * e[0] + info * e[1];
    return e[0] * o0 + e[1] * o1;
}

// NT: a multiple of 64 (the reductions are written for any number of waves; the library instantiates SO_NT)
template <int NT>
__global__ __launch_bounds__(NT) void k_sim3_optimize(const Sim3OptDev *__restrict__ probs, char *__restrict__ ws,
                                                      const float *__restrict__ inv_sigma2, orbm_sim3_opt_result *__restrict__ results)
{
    constexpr int NW = NT / 64;
    __shared__ PairC s_pair[SO_LDS_PAIRS];
    __shared__ Sim3 s_pert[28];                 // [2 d + sign]: Sim3(+-delta e_d) * estimate; [14 + ...]: their inverses
    __shared__ double s_J[14][NT];              // a thread's numeric Jacobian columns of the edge it is working on
    __shared__ double s_red[NW][SO_NSYS];
    __shared__ int s_ired[NW];

    const Sim3OptDev &d = probs[blockIdx.x];
    const int tid = threadIdx.x, n = d.n;
    uint8_t *kept = reinterpret_cast<uint8_t *>(ws + d.o_kept);
    PairC *far = reinterpret_cast<PairC *>(ws + d.o_pair);          // pairs SO_LDS_PAIRS .. n - 1

    Sim3 init;
    sim3_from_rts(d.R12, d.t12, d.s12, init);
    orbm_sim3_opt_result res;
    memset(&res, 0, sizeof(res));
    res.ncorrespondences = n;
    auto store = [&](const Sim3 &S) {
        if (tid != 0) return;
        ORBM_UNROLL for (int k = 0; k < 4; ++k) res.q[k] = S.q[k];
        ORBM_UNROLL for (int k = 0; k < 3; ++k) res.t[k] = S.t[k];
        res.s = S.s;
        results[blockIdx.x] = res;
    };
    if (n <= 0 || n > SO_MAX_N) { store(init); return; }            // no active vertex: optimize() returns -1 (sizes: checked on the host)

    // vPoint1 / vPoint2 (:1501-1511: R * Xw + t as one cv::Mat gemm in float, widened when read), observations, information
    {
        const float *X1 = reinterpret_cast<const float *>(ws + d.o_X1w), *X2 = reinterpret_cast<const float *>(ws + d.o_X2w);
        const float *o1 = reinterpret_cast<const float *>(ws + d.o_obs1), *o2 = reinterpret_cast<const float *>(ws + d.o_obs2);
        const int *l1 = reinterpret_cast<const int *>(ws + d.o_oct1), *l2 = reinterpret_cast<const int *>(ws + d.o_oct2);
        for (int i = tid; i < n; i += NT) {
            PairC c;
            ORBM_UNROLL for (int r = 0; r < 3; ++r) {
                const float a = d.R1[3 * r] * X1[3 * i] + d.R1[3 * r + 1] * X1[3 * i + 1] + d.R1[3 * r + 2] * X1[3 * i + 2];
                const float b = d.R2[3 * r] * X2[3 * i] + d.R2[3 * r + 1] * X2[3 * i + 1] + d.R2[3 * r + 2] * X2[3 * i + 2];
                c.v[r] = (float)((double)a * 1.0 + (double)d.t1[r] * 1.0);
                c.v[3 + r] = (float)((double)b * 1.0 + (double)d.t2[r] * 1.0);
            }
            c.v[6] = o1[2 * i]; c.v[7] = o1[2 * i + 1]; c.v[8] = o2[2 * i]; c.v[9] = o2[2 * i + 1];
            c.v[10] = inv_sigma2[l1[i]]; c.v[11] = inv_sigma2[l2[i]];       // octaves inside [0, nlevels): checked on the host
            if (i < SO_LDS_PAIRS) s_pair[i] = c;
            else far[i - SO_LDS_PAIRS] = c;
            kept[i] = 1;
        }
    }   // (a pair's constants and its kept byte are read by the thread that wrote them: no barrier)
    auto pair = [&](int i) -> PairC { return i < SO_LDS_PAIRS ? s_pair[i] : far[i - SO_LDS_PAIRS]; };

    const float deltaHuber = sqrtf(d.th2);      // :1479
    const double delta_h = deltaHuber, th2 = d.th2;
    const double scalar = 1.0 / (2 * 1e-9);

    // both edges' errors of pair c at S / Sinv
    auto errors = [&](const PairC &c, const Sim3 &S, const Sim3 &Sinv, double e12[2], double e21[2]) {
        const double P1[3] = {c.v[0], c.v[1], c.v[2]}, P2[3] = {c.v[3], c.v[4], c.v[5]};
        const double ob1[2] = {c.v[6], c.v[7]}, ob2[2] = {c.v[8], c.v[9]};
        edge_error(S, P2, ob1, d.cam1, e12);
        edge_error(Sinv, P1, ob2, d.cam2, e21);
    };

    // activeRobustChi2 at T (computeActiveErrors of a trial)
    auto pass_chi = [&](const Sim3 &T) -> double {
        Sim3 Tinv;
        sim3_inverse(T, Tinv);
        double v[1] = {0.0};
        for (int i = tid; i < n; i += NT) {
            if (!kept[i]) continue;
            const PairC c = pair(i);
            double e12[2], e21[2], rho0, w;
            errors(c, T, Tinv, e12, e21);
            huber(edge_chi2((double)c.v[10], e12), delta_h, rho0, w); v[0] += rho0;
            huber(edge_chi2((double)c.v[11], e21), delta_h, rho0, w); v[0] += rho0;
        }
        block_sum<1, NW>(v, s_red);
        return v[0];
    };

    // one edge into the thread's partial system: numeric J (base_binary_edge.hpp:157-173), robust chi2, H += J^T (rho1 omega) J,
    // b += J^T (rho1 * -(omega e)); S0: the estimate or its inverse, pert: the 14 perturbed ones (LDS)
    auto edge_system = [&](const Sim3 &S0, const Sim3 *pert, const double X[3], const double obs[2], const float *cam, double info,
                           double (&v)[SO_NSYS]) {
        double e[2], J0[7], J1[7];
        edge_error(S0, X, obs, cam, e);
        // a rolled loop with the columns parked in the thread's LDS slots: unrolled, the seven pairs of perturbed estimates and their
        // intermediates are all live at once (more than 512 VGPRs, spilled to scratch)
#pragma unroll 1
        for (int dd = 0; dd < 7; ++dd) {
            double ep[2], em[2];
            const Sim3 Sp = pert[2 * dd], Sm = pert[2 * dd + 1];
            edge_error(Sp, X, obs, cam, ep);
            edge_error(Sm, X, obs, cam, em);
            s_J[dd][tid] = scalar * (ep[0] - em[0]);
            s_J[7 + dd][tid] = scalar * (ep[1] - em[1]);
        }
        ORBM_UNROLL for (int dd = 0; dd < 7; ++dd) { J0[dd] = s_J[dd][tid]; J1[dd] = s_J[7 + dd][tid]; }   // (its own thread wrote them: no barrier)
        double rho0, w;
        huber(edge_chi2(info, e), delta_h, rho0, w);
        v[35] += rho0;
        const double winfo = w * info;
        const double r0 = -(info * e[0]) * w, r1 = -(info * e[1]) * w;
        ORBM_UNROLL for (int r = 0; r < 7; ++r) {
            v[28 + r] += J0[r] * r0 + J1[r] * r1;
            ORBM_UNROLL for (int c = 0; c <= r; ++c) v[r * (r + 1) / 2 + c] += J0[r] * (winfo * J0[c]) + J1[r] * (winfo * J1[c]);
        }
    };

    Sim3 est = init, eval = init;               // the estimate; the estimate of the last computeActiveErrors

    // SparseOptimizer::optimize(maxit) over the kept pairs
    auto run_round = [&](int maxit, int &iters, int &trials, double &chi_out) {
        LmStep lm;
        iters = 0; trials = 0;
        for (int iteration = 0; iteration < maxit; ++iteration) {
            ++iters;
            __syncthreads();                                            // the previous iteration's readers are done with s_pert
            if (tid < 14) {
                double u[7] = {0, 0, 0, 0, 0, 0, 0};
                const double step = (tid & 1) ? -1e-9 : 1e-9;
                ORBM_UNROLL for (int k = 0; k < 7; ++k) if ((tid >> 1) == k) u[k] = step;
                if (d.fix_scale) u[6] = 0;                              // oplusImpl, also inside the numeric Jacobian
                Sim3 up, pe, pi;
                sim3_exp(u, up);
                sim3_mul(up, est, pe);
                sim3_inverse(pe, pi);
                s_pert[tid] = pe; s_pert[14 + tid] = pi;
            }
            __syncthreads();
            Sim3 inv;
            sim3_inverse(est, inv);
            double v[SO_NSYS];
            ORBM_UNROLL for (int j = 0; j < SO_NSYS; ++j) v[j] = 0.0;
            for (int i = tid; i < n; i += NT) {
                if (!kept[i]) continue;
                const PairC c = pair(i);
                const double P1[3] = {c.v[0], c.v[1], c.v[2]}, P2[3] = {c.v[3], c.v[4], c.v[5]};
                const double ob1[2] = {c.v[6], c.v[7]}, ob2[2] = {c.v[8], c.v[9]};
                edge_system(est, s_pert, P2, ob1, d.cam1, (double)c.v[10], v);
                edge_system(inv, s_pert + 14, P1, ob2, d.cam2, (double)c.v[11], v);
            }
            block_sum<SO_NSYS, NW>(v, s_red);
            eval = est;
            double currentChi = v[35];
            const double iniChi = currentChi;
            double bb[7];                                               // (H stays packed in v: the lower triangle is all the LDLT reads)
            ORBM_UNROLL for (int r = 0; r < 7; ++r) bb[r] = v[28 + r];
            if (iteration == 0) {                                       // computeLambdaInit, tau = 1e-5
                double maxDiagonal = 0.;
                ORBM_UNROLL for (int j = 0; j < 7; ++j) { const double f = fabs(v[j * (j + 1) / 2 + j]); maxDiagonal = (f < maxDiagonal) ? maxDiagonal : f; }
                lm.start(1e-5 * maxDiagonal);
            }
            double rho = 0;
            int qmax = 0;
            do {
                double Hl[49], x[7] = {0, 0, 0, 0, 0, 0, 0};
                ORBM_UNROLL for (int r = 0; r < 7; ++r)
                    ORBM_UNROLL for (int c = 0; c < 7; ++c) Hl[7 * r + c] = c <= r ? v[r * (r + 1) / 2 + c] : 0.0;
                ORBM_UNROLL for (int j = 0; j < 7; ++j) Hl[8 * j] += lm.lambda;
                const bool ok2 = ldlt_solve<7, LdltZeroDiagonal::AsEigen>(Hl, bb, x);
                if (d.fix_scale) x[6] = 0;                              // oplusImpl writes into the solver's x
                Sim3 up, trial;
                sim3_exp(x, up);
                sim3_mul(up, est, trial);
                double tempChi = pass_chi(trial);
                eval = trial;
                if (!ok2) tempChi = 1.7976931348623157e308;
                double scale = 0.;
                ORBM_UNROLL for (int j = 0; j < 7; ++j) scale += x[j] * (lm.lambda * x[j] + bb[j]);
                rho = lm.verdict(currentChi, tempChi, scale, [&]() { est = trial; }).rho;
                qmax++;
            } while (rho < 0 && qmax < 10);
            trials += qmax;
            chi_out = currentChi;
            if (lm.end_iteration(qmax, rho, iniChi, currentChi) != 1) break;
        }
    };

    // :1570-1587 / :1604-1618: chi2() reads _error of the last TRIED estimate; a NaN is not > th2.  Returns the pairs cut here.
    auto cut = [&]() -> int {
        Sim3 einv;
        sim3_inverse(eval, einv);
        int bad = 0;
        for (int i = tid; i < n; i += NT) {
            if (!kept[i]) continue;
            const PairC c = pair(i);
            double e12[2], e21[2];
            errors(c, eval, einv, e12, e21);
            if (edge_chi2((double)c.v[10], e12) > th2 || edge_chi2((double)c.v[11], e21) > th2) { kept[i] = 0; bad++; }
        }
        return block_sum_int<NW>(bad, s_ired);
    };

    int nBad = 0;
    for (int round = 0; round < 2; ++round) {
        int it = 0, tr = 0;
        double chi = 0.0;
        run_round(round == 0 ? 5 : (nBad > 0 ? 10 : 5), it, tr, chi);
        if (round == 0) { res.iterations[0] = it; res.trials[0] = tr; }
        else { res.iterations[1] = it; res.trials[1] = tr; }
        res.chi2 = chi;
        const int c = cut();
        if (round == 0) {
            res.nbad = nBad = c;
            if (n - nBad < 10) { store(init); return; }                // :1595: g2oS12 stays as it came in
        } else res.nin = n - nBad - c;
    }
    store(est);
}

std::atomic<int> g_last_sim3_opt_waits{0};     // host waits of the last orbm_optimize_sim3 call of this process

} // namespace

void orbm_detail::launch_sim3_optimize(hipStream_t st, const Sim3OptDev *dprobs, int P, char *ws, const float *dinv_sigma2,
                                       orbm_sim3_opt_result *dresults)
{
    hipLaunchKernelGGL(k_sim3_optimize<SO_NT>, dim3((unsigned)P), dim3(SO_NT), 0, st, dprobs, ws, dinv_sigma2, dresults);
}

void orbm_detail::sim3_opt_empty_result(const float *R12, const float *t12, float s12, orbm_sim3_opt_result &r)
{
    memset(&r, 0, sizeof(r));
    Sim3 S;
    sim3_from_rts(R12, t12, s12, S);
    for (int k = 0; k < 4; ++k) r.q[k] = S.q[k];
    for (int k = 0; k < 3; ++k) r.t[k] = S.t[k];
    r.s = S.s;
}

extern "C" {

int orbm_optimize_sim3(const orbm_sim3_opt_problem *problems, int P, const float *inv_level_sigma2, int nlevels,
                       orbm_sim3_opt_result *results, uint8_t *kept)
{
    g_last_sim3_opt_waits.store(0, std::memory_order_relaxed);
    if (P < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (P > SO_MAX_P) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 64 problems in one call");
    if (P && (!problems || !results)) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    size_t total = 0;
    for (int p = 0; p < P; ++p) {
        const orbm_sim3_opt_problem &q = problems[p];
        if (q.n < 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        if (q.n > SO_MAX_N) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 8,192 correspondences in a problem");
        if (q.n == 0) continue;
        if (!q.X1w || !q.X2w || !q.obs1 || !q.obs2 || !q.octave1 || !q.octave2 || !q.Tcw1 || !q.Tcw2 || !inv_level_sigma2 || nlevels < 1 || !kept)
            ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
        if (!octaves_in_range(q, nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
        total += (size_t)q.n;
    }
    for (int p = 0; p < P; ++p) sim3_opt_empty_result(problems[p].R12, problems[p].t12, problems[p].s12, results[p]);
    if (total == 0) return ORBX_OK;
    ORBX_NEED_DEVICE();
    std::vector<Sim3OptDev> dev((size_t)P);
    StagedCall sc;
    const size_t o_dev = sc.in(dev.data(), sizeof(Sim3OptDev) * (size_t)P), o_sg = sc.in(inv_level_sigma2, sizeof(float) * (size_t)nlevels);
    for (int p = 0; p < P; ++p) {
        const orbm_sim3_opt_problem &q = problems[p];
        Sim3OptDev &d = dev[p];
        memset(&d, 0, sizeof(d));
        d.n = q.n; d.fix_scale = q.fix_scale ? 1 : 0; d.th2 = q.th2; d.s12 = q.s12;
        memcpy(d.R12, q.R12, sizeof(d.R12)); memcpy(d.t12, q.t12, sizeof(d.t12));
        if (q.n == 0) continue;
        stage_two_keyframes(sc, q, d);
        const size_t n = (size_t)q.n;
        d.o_obs1 = (unsigned)sc.in(q.obs1, sizeof(float) * 2 * n); d.o_obs2 = (unsigned)sc.in(q.obs2, sizeof(float) * 2 * n);
    }
    for (int p = 0; p < P; ++p)
        if (dev[p].n > SO_LDS_PAIRS) dev[p].o_pair = (unsigned)sc.scratch(sizeof(PairC) * (size_t)(dev[p].n - SO_LDS_PAIRS));
    const size_t o_res = sc.out(sizeof(orbm_sim3_opt_result) * (size_t)P);
    for (int p = 0; p < P; ++p)
        if (dev[p].n) dev[p].o_kept = (unsigned)sc.out((size_t)dev[p].n);
    if (!sc.offsets_fit_32_bits()) ORBX_FAIL(ORBX_ERR_CAPACITY, "the call's arrays exceed 4 GiB");
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    launch_sim3_optimize(sc.stream(), sc.d<const Sim3OptDev>(o_dev), P, sc.d<char>(0), sc.d<const float>(o_sg), sc.d<orbm_sim3_opt_result>(o_res));
    ORBX_HIP(hipGetLastError());
    const int drc = sc.download();
    g_last_sim3_opt_waits.store(sc.waits, std::memory_order_relaxed);  // counted where the stream is waited for
    if (drc) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(results, sc.r<orbm_sim3_opt_result>(o_res), sizeof(orbm_sim3_opt_result) * (size_t)P);
    uint8_t *out = kept;
    for (int p = 0; p < P; ++p) {
        if (dev[p].n) memcpy(out, sc.r<uint8_t>(dev[p].o_kept), (size_t)dev[p].n);
        out += dev[p].n;
    }
    return ORBX_OK;
}

int orbm_debug_last_sim3_opt_waits(void) { return g_last_sim3_opt_waits.load(std::memory_order_relaxed); }

} // extern "C"
