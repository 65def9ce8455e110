/* Prints the C layout of orbm_init_models and orbm_init_reconstruction for tests/test_cpu_init.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_init_models);
    F(orbm_init_models, H21); F(orbm_init_models, F21); F(orbm_init_models, SH); F(orbm_init_models, SF);
    F(orbm_init_models, itH); F(orbm_init_models, itF);
    S(orbm_init_reconstruction);
    F(orbm_init_reconstruction, R21); F(orbm_init_reconstruction, t21); F(orbm_init_reconstruction, parallax);
    F(orbm_init_reconstruction, ngood); F(orbm_init_reconstruction, found); F(orbm_init_reconstruction, best);
    F(orbm_init_reconstruction, N); F(orbm_init_reconstruction, max_good); F(orbm_init_reconstruction, nsimilar);
    return 0;
}
