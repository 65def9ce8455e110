/* Prints the C layout of orbm_triang_keyframe for tests/test_cpu_create_points.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_triang_keyframe);
    F(orbm_triang_keyframe, frame); F(orbm_triang_keyframe, Tcw);
    F(orbm_triang_keyframe, fx); F(orbm_triang_keyframe, fy); F(orbm_triang_keyframe, cx); F(orbm_triang_keyframe, cy);
    F(orbm_triang_keyframe, invfx); F(orbm_triang_keyframe, invfy); F(orbm_triang_keyframe, mb); F(orbm_triang_keyframe, mbf);
    F(orbm_triang_keyframe, depth); F(orbm_triang_keyframe, has_mappoint);
    F(orbm_triang_keyframe, nodes); F(orbm_triang_keyframe, off); F(orbm_triang_keyframe, items); F(orbm_triang_keyframe, nn);
    F(orbm_triang_keyframe, F12); F(orbm_triang_keyframe, ex); F(orbm_triang_keyframe, ey);
    printf("enum ORBM_TRI_NO_MATCH %d\nenum ORBM_TRI_CREATED %d\nenum ORBM_TRI_SKIPPED %d\nenum ORBM_TRI_SVD_ZERO %d\n", ORBM_TRI_NO_MATCH,
           ORBM_TRI_CREATED, ORBM_TRI_SKIPPED, ORBM_TRI_SVD_ZERO);
    printf("enum ORBM_TRI_PARALLAX %d\nenum ORBM_TRI_DEPTH %d\nenum ORBM_TRI_REPROJ1 %d\nenum ORBM_TRI_REPROJ2 %d\n", ORBM_TRI_PARALLAX,
           ORBM_TRI_DEPTH, ORBM_TRI_REPROJ1, ORBM_TRI_REPROJ2);
    printf("enum ORBM_TRI_DIST_ZERO %d\nenum ORBM_TRI_SCALE %d\nenum ORBM_TRI_NSTATUS %d\n", ORBM_TRI_DIST_ZERO, ORBM_TRI_SCALE, ORBM_TRI_NSTATUS);
    return 0;
}
