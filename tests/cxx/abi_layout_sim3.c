/* Prints the C layout of orbm_sim3_problem and orbm_sim3_hypothesis for tests/test_cpu_sim3.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_sim3_problem);
    F(orbm_sim3_problem, X1w); F(orbm_sim3_problem, X2w); F(orbm_sim3_problem, octave1); F(orbm_sim3_problem, octave2);
    F(orbm_sim3_problem, Tcw1); F(orbm_sim3_problem, Tcw2);
    F(orbm_sim3_problem, fx1); F(orbm_sim3_problem, fy1); F(orbm_sim3_problem, cx1); F(orbm_sim3_problem, cy1);
    F(orbm_sim3_problem, fx2); F(orbm_sim3_problem, fy2); F(orbm_sim3_problem, cx2); F(orbm_sim3_problem, cy2);
    F(orbm_sim3_problem, triples); F(orbm_sim3_problem, n); F(orbm_sim3_problem, H); F(orbm_sim3_problem, fix_scale);
    S(orbm_sim3_hypothesis);
    F(orbm_sim3_hypothesis, T12); F(orbm_sim3_hypothesis, R12); F(orbm_sim3_hypothesis, t12); F(orbm_sim3_hypothesis, s12);
    F(orbm_sim3_hypothesis, ninliers);
    return 0;
}
