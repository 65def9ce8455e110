// orbm_levenberg.h -- the step rule of g2o's OptimizationAlgorithmLevenberg::solve (Thirdparty/g2o/g2o/core/
// optimization_algorithm_levenberg.cpp:63-241), the one copy of it: the three kernels that run the whole loop (orbm_pose.hip,
// orbm_sim3opt.hip, orbm_pose_nr.hip) and the host loop that steps kernels (LmHostLoop::trials, orbm_internal.h: orbm_ba.hip,
// orbm_essential_graph.hip) all take their decisions here.  What stays with a solver: the largest diagonal entry behind lambda's
// first value, the trial loop's condition (rho < 0 && qmax < 10), push / pop of its estimates, and whatever it does to tempChi
// before the verdict; push / pop ride in the verdict's one branch as the caller's callables (a second branch on the decision behind
// it costs k_pose_nr its instruction stream).  Plain scalars and inline functions: in a kernel the state lives in registers.  A plain C++ compiler takes the file
// too (tests/cxx/levenberg_rule.cpp drives it against a restatement).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORBM_LM_FN __host__ __device__ __forceinline__
#else
#define ORBM_LM_FN inline
#endif

namespace orbm_detail {

struct LmVerdict {
    double rho, scale;          // scale: with the + 1e-3
    bool accepted;
};

struct LmNothing { ORBM_LM_FN void operator()() const {} };

struct LmStep {
    double lambda = -1., ni = 2.;   // _currentLambda, _ni (levenberg.cpp:46-57)
    int lmBad = 0;                  // _nBad

    // iteration 0 of an optimize() call (:97-115); lambda_init: computeLambdaInit's value, tau * the largest diagonal entry or the user's
    ORBM_LM_FN void start(double lambda_init)
    {
        lambda = lambda_init;
        ni = 2;
        lmBad = 0;
    }

    // One trial (:201-223).  tempChi: the trial's robust chi2, DBL_MAX when the solve failed; scale: computeScale's sum.  An accepted
    // trial's tempChi becomes currentChi.  on_accept() / on_reject(): what the caller does with its estimates (discardTop / pop),
    // inside the rule's own branch.
    template <class Accept = LmNothing, class Reject = LmNothing>
    ORBM_LM_FN LmVerdict verdict(double &currentChi, double tempChi, double scale, Accept &&on_accept = Accept(), Reject &&on_reject = Reject())
    {
        double rho = (currentChi - tempChi);
        scale += 1e-3;
        rho /= scale;
        const bool good = rho > 0 && std::isfinite(tempChi);
        if (good) {
            double alpha = 1. - pow((2 * rho - 1), 3.0);
            alpha = (alpha < 2. / 3.) ? alpha : 2. / 3.;
            const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;
            lambda *= scaleFactor;
            ni = 2;
            currentChi = tempChi;
            on_accept();
        } else {
            lambda *= ni;
            ni *= 2;
            on_reject();
        }
        return {rho, scale, good};
    }

    // Behind the trial loop (:228-239): the SolverResult, 1 OK or 2 Terminate (sparse_optimizer.cpp:470 leaves on anything but OK)
    ORBM_LM_FN int end_iteration(int qmax, double rho, double iniChi, double currentChi)
    {
        if (qmax == 10 || rho == 0) return 2;
        if ((iniChi - currentChi) * 1e3 < iniChi) lmBad++;      // Raul's stop criterion
        else lmBad = 0;
        return lmBad >= 3 ? 2 : 1;
    }
};

} // namespace orbm_detail
