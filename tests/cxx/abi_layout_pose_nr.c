/* Prints the C layout of orbm_pose_nr_graph, orbm_pose_nr_result, orbm_pose_nr_trial and orbm_pose_nr_stats for
 * tests/test_cpu_pose_nr_bundle.py: "struct <name> <size>", then one "field <struct> <name> <offset> <width>" per member, in
 * declaration order (the format of abi_layout.c). */
#include <stddef.h>
#include <stdio.h>

#include "fem_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_pose_nr_graph);
    F(orbm_pose_nr_graph, npoints); F(orbm_pose_nr_graph, nkf); F(orbm_pose_nr_graph, nedges); F(orbm_pose_nr_graph, reserved);
    F(orbm_pose_nr_graph, Tcw); F(orbm_pose_nr_graph, kf_Tcw); F(orbm_pose_nr_graph, points); F(orbm_pose_nr_graph, e_point);
    F(orbm_pose_nr_graph, e_cam); F(orbm_pose_nr_graph, e_obs); F(orbm_pose_nr_graph, e_inv_sigma2); F(orbm_pose_nr_graph, e_cam_k);
    S(orbm_pose_nr_result);
    F(orbm_pose_nr_result, Tcw); F(orbm_pose_nr_result, points_out); F(orbm_pose_nr_result, outlier); F(orbm_pose_nr_result, ngood);
    F(orbm_pose_nr_result, reserved);
    S(orbm_pose_nr_trial);
    F(orbm_pose_nr_trial, sE); F(orbm_pose_nr_trial, nsE); F(orbm_pose_nr_trial, tempChi); F(orbm_pose_nr_trial, currentChi);
    F(orbm_pose_nr_trial, rho); F(orbm_pose_nr_trial, lambda); F(orbm_pose_nr_trial, qmax); F(orbm_pose_nr_trial, accepted);
    S(orbm_pose_nr_stats);
    F(orbm_pose_nr_stats, rounds); F(orbm_pose_nr_stats, iterations); F(orbm_pose_nr_stats, trials); F(orbm_pose_nr_stats, nresults);
    F(orbm_pose_nr_stats, results); F(orbm_pose_nr_stats, trial_capacity); F(orbm_pose_nr_stats, ntrials);
    F(orbm_pose_nr_stats, trial_overflow); F(orbm_pose_nr_stats, reserved); F(orbm_pose_nr_stats, trial_log); F(orbm_pose_nr_stats, q);
    F(orbm_pose_nr_stats, t); F(orbm_pose_nr_stats, points);
    return 0;
}
