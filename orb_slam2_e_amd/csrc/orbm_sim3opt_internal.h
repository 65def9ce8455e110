// orbm_sim3opt_internal.h -- what orbm_sim3opt.hip (orbm_optimize_sim3) and orbm_refine_sim3.hip (orbm_refine_sim3_candidates) share:
// the device record of one OptimizeSim3 problem, the kernel's limits and its launch.  The kernel itself, k_sim3_optimize, exists
// once, in orbm_sim3opt.hip.
#pragma once
#include "orbm_internal.h"

namespace orbm_detail {

constexpr int SO_MAX_P = 64, SO_MAX_N = 8192;
constexpr int SO_LDS_PAIRS = 512;       // pairs whose constants are staged in LDS (48 B each)
constexpr size_t SO_PAIR_BYTES = 48;    // sizeof(PairC): a pair's constants behind the LDS-staged ones, in the o_pair scratch

// One problem of a call, staged with the inputs.  o_*: byte offsets in the workspace.
struct Sim3OptDev {
    unsigned o_X1w, o_X2w, o_obs1, o_obs2, o_oct1, o_oct2;          // the pairs: staged inputs (orbm_optimize_sim3) or k_refine_gather's output
    unsigned o_pair;                                                 // scratch: the constants of the pairs behind the LDS-staged ones
    unsigned o_kept;                                                 // result: [n] bytes
    int n, fix_scale;                                                // (n: from the host, or written by k_refine_gather in front of the launch)
    float th2, s12;
    float R1[9], t1[3], R2[9], t2[3];                                // Tcw1, Tcw2
    float cam1[4], cam2[4];                                          // fx, fy, cx, cy
    float R12[9], t12[3];
};

// k_sim3_optimize over P records in device memory: problem p's result into results[p], its kept bytes at o_kept
void launch_sim3_optimize(hipStream_t st, const Sim3OptDev *dprobs, int P, char *ws, const float *dinv_sigma2, orbm_sim3_opt_result *dresults);

// what a problem without a correspondence returns (Optimizer.cc:1595 with nothing optimised): the input Sim3, every count 0
void sim3_opt_empty_result(const float *R12, const float *t12, float s12, orbm_sim3_opt_result &r);

} // namespace orbm_detail
