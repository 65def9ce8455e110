/* The C layout of orbm_track_result, read by tests/test_cpu_track.py: the line format of abi_layout.c. */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("field %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))

int main(void)
{
    S(orbm_track_result);
    F(orbm_track_result, tracked); F(orbm_track_result, search_used); F(orbm_track_result, nsearch); F(orbm_track_result, ngood);
    F(orbm_track_result, nmatches); F(orbm_track_result, nmatches_map);
    return 0;
}
