/* Prints the C layout of orbm_pnp_problem and orbm_pnp_hypothesis for tests/test_cpu_pnp.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_pnp_problem);
    F(orbm_pnp_problem, Xw); F(orbm_pnp_problem, uv); F(orbm_pnp_problem, octave); F(orbm_pnp_problem, sets);
    F(orbm_pnp_problem, fu); F(orbm_pnp_problem, fv); F(orbm_pnp_problem, uc); F(orbm_pnp_problem, vc);
    F(orbm_pnp_problem, th2); F(orbm_pnp_problem, n); F(orbm_pnp_problem, H); F(orbm_pnp_problem, min_inliers);
    S(orbm_pnp_hypothesis);
    F(orbm_pnp_hypothesis, R); F(orbm_pnp_hypothesis, t); F(orbm_pnp_hypothesis, rep_error); F(orbm_pnp_hypothesis, ninliers);
    F(orbm_pnp_hypothesis, refined); F(orbm_pnp_hypothesis, Rr); F(orbm_pnp_hypothesis, tr); F(orbm_pnp_hypothesis, nrefined);
    F(orbm_pnp_hypothesis, pad);
    return 0;
}
