/* Prints the C layout of orbm_ba_graph, orbm_ba_options, orbm_ba_result, orbm_ba_trial and orbm_ba_stats for tests/test_cpu_ba.py:
 * "struct <name> <size>", then one "field <struct> <name> <offset> <width>" per member, in declaration order (the format of
 * abi_layout.c); then the two documented initialisers as "options <name> <the nine values>". */
#include <stddef.h>
#include <stdio.h>

#include "orbslam_hip.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

static void options(const char *name, const orbm_ba_options *o)
{
    printf("options %s %d %d %d %d %d %.17g %.17g %.17g %.17g\n", name, o->nrounds, o->iterations[0], o->iterations[1], o->robust_round0,
           o->classify, o->huber_mono, o->huber_stereo, o->chi2_mono, o->chi2_stereo);
}

int main(void)
{
    S(orbm_ba_graph);
    F(orbm_ba_graph, nfree); F(orbm_ba_graph, nfixed); F(orbm_ba_graph, npoints); F(orbm_ba_graph, nedges); F(orbm_ba_graph, poses);
    F(orbm_ba_graph, fixed); F(orbm_ba_graph, points); F(orbm_ba_graph, e_point); F(orbm_ba_graph, e_cam); F(orbm_ba_graph, e_obs);
    F(orbm_ba_graph, e_inv_sigma2); F(orbm_ba_graph, e_cam_k);
    S(orbm_ba_options);
    F(orbm_ba_options, nrounds); F(orbm_ba_options, iterations); F(orbm_ba_options, robust_round0); F(orbm_ba_options, classify);
    F(orbm_ba_options, reserved); F(orbm_ba_options, huber_mono); F(orbm_ba_options, huber_stereo); F(orbm_ba_options, chi2_mono);
    F(orbm_ba_options, chi2_stereo);
    S(orbm_ba_result);
    F(orbm_ba_result, poses); F(orbm_ba_result, points); F(orbm_ba_result, erase); F(orbm_ba_result, not_included); F(orbm_ba_result, stopped);
    S(orbm_ba_trial);
    F(orbm_ba_trial, tempChi); F(orbm_ba_trial, currentChi); F(orbm_ba_trial, rho); F(orbm_ba_trial, lambda); F(orbm_ba_trial, scale);
    F(orbm_ba_trial, round); F(orbm_ba_trial, qmax); F(orbm_ba_trial, accepted); F(orbm_ba_trial, ok2);
    S(orbm_ba_stats);
    F(orbm_ba_stats, rounds); F(orbm_ba_stats, iterations); F(orbm_ba_stats, trials); F(orbm_ba_stats, nresults); F(orbm_ba_stats, results);
    F(orbm_ba_stats, trial_capacity); F(orbm_ba_stats, ntrials); F(orbm_ba_stats, trial_overflow); F(orbm_ba_stats, trial_log);
    F(orbm_ba_stats, poses); F(orbm_ba_stats, points); F(orbm_ba_stats, chi2); F(orbm_ba_stats, level);
    {
        const orbm_ba_options local = ORBM_BA_OPTIONS_LOCAL, global = ORBM_BA_OPTIONS_GLOBAL(20, 0);
        options("local", &local);
        options("global", &global);
    }
    return 0;
}
