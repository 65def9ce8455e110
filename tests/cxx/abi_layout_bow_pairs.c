/* Prints the C layout of orbm_bow_pair for tests/test_cpu_bow_pairs.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_bow_pair);
    F(orbm_bow_pair, frame1); F(orbm_bow_pair, nodes1); F(orbm_bow_pair, off1); F(orbm_bow_pair, items1); F(orbm_bow_pair, nn1);
    F(orbm_bow_pair, valid1);
    F(orbm_bow_pair, frame2); F(orbm_bow_pair, nodes2); F(orbm_bow_pair, off2); F(orbm_bow_pair, items2); F(orbm_bow_pair, nn2);
    F(orbm_bow_pair, valid2);
    F(orbm_bow_pair, match12); F(orbm_bow_pair, match21);
    return 0;
}
