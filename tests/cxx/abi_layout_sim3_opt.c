/* Prints the C layout of orbm_sim3_opt_problem and orbm_sim3_opt_result for tests/test_cpu_sim3_opt.py: "struct <name> <size>", then
 * one "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_sim3_opt_problem);
    F(orbm_sim3_opt_problem, X1w); F(orbm_sim3_opt_problem, X2w); F(orbm_sim3_opt_problem, obs1); F(orbm_sim3_opt_problem, obs2);
    F(orbm_sim3_opt_problem, octave1); F(orbm_sim3_opt_problem, octave2); F(orbm_sim3_opt_problem, Tcw1); F(orbm_sim3_opt_problem, Tcw2);
    F(orbm_sim3_opt_problem, fx1); F(orbm_sim3_opt_problem, fy1); F(orbm_sim3_opt_problem, cx1); F(orbm_sim3_opt_problem, cy1);
    F(orbm_sim3_opt_problem, fx2); F(orbm_sim3_opt_problem, fy2); F(orbm_sim3_opt_problem, cx2); F(orbm_sim3_opt_problem, cy2);
    F(orbm_sim3_opt_problem, R12); F(orbm_sim3_opt_problem, t12); F(orbm_sim3_opt_problem, s12); F(orbm_sim3_opt_problem, th2);
    F(orbm_sim3_opt_problem, fix_scale); F(orbm_sim3_opt_problem, n);
    S(orbm_sim3_opt_result);
    F(orbm_sim3_opt_result, q); F(orbm_sim3_opt_result, t); F(orbm_sim3_opt_result, s); F(orbm_sim3_opt_result, nin);
    F(orbm_sim3_opt_result, nbad); F(orbm_sim3_opt_result, ncorrespondences); F(orbm_sim3_opt_result, iterations);
    F(orbm_sim3_opt_result, trials); F(orbm_sim3_opt_result, chi2);
    return 0;
}
