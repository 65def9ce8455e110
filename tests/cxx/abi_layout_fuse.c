/* Prints the C layout of orbm_fuse_target and orbm_camera for tests/test_cpu_fuse_keyframes.py: "struct <name> <size>", then one
 * "field <struct> <name> <offset> <width>" per member, in declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_fuse_target);
    F(orbm_fuse_target, frame); F(orbm_fuse_target, Rcw); F(orbm_fuse_target, tcw); F(orbm_fuse_target, Ow);
    F(orbm_fuse_target, cam); F(orbm_fuse_target, mbf);
    S(orbm_camera);
    F(orbm_camera, fx); F(orbm_camera, fy); F(orbm_camera, cx); F(orbm_camera, cy);
    F(orbm_camera, min_x); F(orbm_camera, max_x); F(orbm_camera, min_y); F(orbm_camera, max_y);
    F(orbm_camera, grid_min_x); F(orbm_camera, grid_min_y); F(orbm_camera, grid_max_x); F(orbm_camera, grid_max_y);
    return 0;
}
