/* Prints the C layout of orbm_refine_sim3_attempt for tests/test_cpu_refine_sim3.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_refine_sim3_attempt);
    F(orbm_refine_sim3_attempt, kf2); F(orbm_refine_sim3_attempt, points2); F(orbm_refine_sim3_attempt, T2w);
    F(orbm_refine_sim3_attempt, R12); F(orbm_refine_sim3_attempt, t12); F(orbm_refine_sim3_attempt, s12);
    F(orbm_refine_sim3_attempt, seed12); F(orbm_refine_sim3_attempt, found12); F(orbm_refine_sim3_attempt, matches12);
    return 0;
}
