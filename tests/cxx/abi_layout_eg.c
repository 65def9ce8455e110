/* Prints the C layout of orbm_eg_graph, orbm_eg_options, orbm_eg_result and orbm_eg_stats for tests/test_cpu_essential_graph.py:
 * "struct <name> <size>", then one "field <struct> <name> <offset> <width>" per member, in declaration order (the format of
 * abi_layout.c); then the documented initialiser as "options default <the three values>". */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main(void)
{
    S(orbm_eg_graph);
    F(orbm_eg_graph, nvert); F(orbm_eg_graph, ncorr); F(orbm_eg_graph, nnc); F(orbm_eg_graph, nedges); F(orbm_eg_graph, npoints);
    F(orbm_eg_graph, fix_scale); F(orbm_eg_graph, poses); F(orbm_eg_graph, corrected); F(orbm_eg_graph, corrected_sim3);
    F(orbm_eg_graph, noncorrected); F(orbm_eg_graph, noncorrected_sim3); F(orbm_eg_graph, fixed); F(orbm_eg_graph, e_v0); F(orbm_eg_graph, e_v1);
    F(orbm_eg_graph, e_kind); F(orbm_eg_graph, points); F(orbm_eg_graph, p_ref);
    S(orbm_eg_options);
    F(orbm_eg_options, iterations); F(orbm_eg_options, reserved); F(orbm_eg_options, lambda_init);
    S(orbm_eg_result);
    F(orbm_eg_result, poses); F(orbm_eg_result, points);
    S(orbm_eg_stats);
    F(orbm_eg_stats, iterations); F(orbm_eg_stats, trials); F(orbm_eg_stats, nresults); F(orbm_eg_stats, results); F(orbm_eg_stats, trial_capacity);
    F(orbm_eg_stats, ntrials); F(orbm_eg_stats, trial_overflow); F(orbm_eg_stats, trial_log); F(orbm_eg_stats, estimates); F(orbm_eg_stats, chi2);
    S(orbm_ba_trial);
    {
        const orbm_eg_options o = ORBM_EG_OPTIONS_DEFAULT;
        printf("options default %d %d %.17g\n", o.iterations, o.reserved, o.lambda_init);
    }
    return 0;
}
