/* Prints the C layout of orbm_distortion for tests/test_cpu_undistort.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_distortion);
    F(orbm_distortion, fx); F(orbm_distortion, fy); F(orbm_distortion, cx); F(orbm_distortion, cy);
    F(orbm_distortion, k1); F(orbm_distortion, k2); F(orbm_distortion, p1); F(orbm_distortion, p2); F(orbm_distortion, k3);
    return 0;
}
