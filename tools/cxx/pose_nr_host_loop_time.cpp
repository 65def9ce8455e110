// Times the host-driven form of PoseOptimizationNR's bundle for tools/pose_nr_time.py: orbslam_hip::PoseOptimizationNR_fem::Optimize
// over the mini-g2o graph (oracle/mini_g2o.h), one fem_trial_energy call per Levenberg trial.  The model is built once; every timed
// run restarts from the scene's estimates.  usage: pose_nr_host_loop_time <scene.bin> <batches> <calls>; the scene format is
// tests/cxx/pose_nr_lm.cpp's.  Prints one line: the mean milliseconds of a run per batch, then the trials of a run.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"
#include "../../oracle/mini_g2o.h"

using namespace orbslam_hip;

struct MiniG2O {
    mg_problem *g;
    void initializeOptimization(int) { mg_initialize_optimization(g); }
    double activeRobustChi2() { return mg_active_robust_chi2(g); }
    void buildSystem() { mg_build_system(g); }
    double computeLambdaInit() { return mg_lambda_init(g); }
    void push() { mg_push(g); }
    void pop() { mg_pop(g); }
    void discardTop() {}
    bool solveAndUpdate(double lambda) { return mg_solve_and_update(g, lambda) != 0; }
    double computeScale(double lambda) { return mg_compute_scale(g, lambda); }
    void pointEstimates(std::vector<double> &xyz) { xyz.assign(g->X, g->X + 3 * (size_t)g->npts); }
    bool terminate() { return false; }
    void classifyOutliers(int) { mg_classify_outliers(g); }
};

template <class T> static void rd(FILE *f, T *v, size_t n)
{
    if (n && fread(v, sizeof(T), n, f) != n) { fprintf(stderr, "short scene\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int nbatch = atoi(argv[2]), ncalls = atoi(argv[3]);
    int32_t hd[7]; rd(f, hd, 7);
    const int nElType = hd[0], nTop = hd[1], nFaces = hd[2], nVertices = hd[3], nDerived = hd[4], nKF = hd[5], nEdges = hd[6];
    std::vector<float> top((size_t)3 * nTop); rd(f, top.data(), top.size());
    std::vector<int32_t> faces((size_t)(nElType == 1 ? 4 : 3) * nFaces); rd(f, faces.data(), faces.size());
    std::vector<int32_t> derived((size_t)4 * nDerived); rd(f, derived.data(), derived.size());
    mg_problem *g = mg_create(nVertices, nKF, nEdges);
    rd(f, g->R, 9); rd(f, g->t, 3); rd(f, g->kfR, (size_t)9 * nKF); rd(f, g->kft, (size_t)3 * nKF); rd(f, g->X, (size_t)3 * nVertices);
    rd(f, g->e_pt, nEdges); rd(f, g->e_cam, nEdges); rd(f, g->e_obs, (size_t)2 * nEdges); rd(f, g->e_info, nEdges); rd(f, g->e_K, (size_t)4 * nEdges);
    fclose(f);
    double R0[9], t0[3];
    memcpy(R0, g->R, sizeof(R0)); memcpy(t0, g->t, sizeof(t0));
    const std::vector<double> X0(g->X, g->X + 3 * (size_t)nVertices);

    PoseOptimizationNR_fem nr(nElType);
    if (!nr.Compute(top, faces, nVertices, derived)) { fprintf(stderr, "Compute(1) failed: %d %s\n", nr.status(), orbx_last_error()); return 1; }
    MiniG2O g2o{g};
    size_t trials = 0;
    auto run = [&]() {
        memcpy(g->R, R0, sizeof(R0)); memcpy(g->t, t0, sizeof(t0)); memcpy(g->X, X0.data(), sizeof(double) * X0.size());
        memset(g->e_level, 0, sizeof(int) * nEdges); memset(g->outlier, 0, nVertices); memset(g->reloc_check, 1, nVertices);
        std::vector<PoseOptimizationNR_fem::Trial> log;
        nr.Optimize(g2o, &log, nullptr);
        trials = log.size();
    };
    run();                                                              // warm-up
    if (nr.status() != ORBX_OK) { fprintf(stderr, "status %d %s\n", nr.status(), orbx_last_error()); return 1; }
    for (int b = 0; b < nbatch; ++b) {
        const auto t0c = std::chrono::steady_clock::now();
        for (int c = 0; c < ncalls; ++c) run();
        printf("%.4f ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0c).count() / ncalls);
    }
    printf("%zu\n", trials);
    return 0;
}
