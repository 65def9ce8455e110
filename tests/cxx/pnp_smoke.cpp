// orbslam_hip::PnPsolver (include/orbslam_hip.hpp) from C++, built and run by tests/test_cpu_pnp.py and tests/test_gpu_pnp.py.
// Every argument is a scene file written by the test (tests/pnp_scenes.py data with pre-drawn sets):
//   n nMatches H fu fv uc vc minInliers maxIterations ncalls, the ncalls values of nIterations, nlevels, mvLevelSigma2,
//   n rows "X Y Z u v octave index", H rows of four set indices
// One solver per file; PnPsolver::evaluate runs the first evaluation of all of them in ONE library call, then every solver makes
// its iterate calls, printed as "call <file> <found> <bNoMore> <nInliers> <Tcw as 16 hex words> : <the set vbInliers places>".
// argv[1] = "nodevice": expect the first iterate of the one scene that follows to fail loudly.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "orbslam_hip.hpp"

using orbslam_hip::PnPsolver;

struct Scene {
    PnPsolver::Problem p;
    std::vector<int32_t> sets;
    std::vector<int> calls;
    int minInliers = 8, maxIterations = 300;
};

static bool load(const char *path, Scene &s)
{
    FILE *f = fopen(path, "r");
    if (!f) return false;
    int n, H, ncalls;
    bool ok = fscanf(f, "%d %d %d %lf %lf %lf %lf %d %d %d", &n, &s.p.nMatches, &H, &s.p.fu, &s.p.fv, &s.p.uc, &s.p.vc, &s.minInliers, &s.maxIterations,
                     &ncalls) == 10;
    for (int k = 0; ok && k < ncalls; ++k) { int c; ok = fscanf(f, "%d", &c) == 1; s.calls.push_back(c); }
    int nlevels = 0;
    ok = ok && fscanf(f, "%d", &nlevels) == 1;
    for (int l = 0; ok && l < nlevels; ++l) { float v; ok = fscanf(f, "%f", &v) == 1; s.p.levelSigma2.push_back(v); }
    for (int i = 0; ok && i < n; ++i) {
        float v[5];
        int oct, idx;
        ok = fscanf(f, "%f %f %f %f %f %d %d", v, v + 1, v + 2, v + 3, v + 4, &oct, &idx) == 7;
        s.p.Xw.insert(s.p.Xw.end(), v, v + 3); s.p.uv.insert(s.p.uv.end(), v + 3, v + 5);
        s.p.octave.push_back(oct); s.p.indices.push_back(idx);
    }
    for (int k = 0; ok && k < 4 * H; ++k) { int v; ok = fscanf(f, "%d", &v) == 1; s.sets.push_back(v); }
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    const bool nodevice = argc > 1 && !strcmp(argv[1], "nodevice");
    std::vector<Scene> scenes;
    for (int a = nodevice ? 2 : 1; a < argc; ++a) {
        Scene s;
        if (!load(argv[a], s)) { printf("FAIL cannot read %s\n", argv[a]); return 1; }
        scenes.push_back(s);
    }
    if (scenes.empty()) { printf("FAIL no scene\n"); return 1; }
    std::vector<std::unique_ptr<PnPsolver> > solvers;
    std::vector<PnPsolver *> all;
    for (Scene &s : scenes) {
        solvers.emplace_back(new PnPsolver(s.p, s.sets));
        solvers.back()->SetRansacParameters(0.99, s.minInliers, s.maxIterations);
        all.push_back(solvers.back().get());
    }
    std::vector<bool> inl;
    int nin = -1;
    bool noMore = false;
    float T[16];
    if (nodevice) {
        PnPsolver &a = *all[0];
        const bool found = a.iterate(5, noMore, inl, nin, T);
        if (found || a.status() != ORBX_ERR_NO_DEVICE || !noMore || nin != 0 || (int)inl.size() != scenes[0].p.nMatches) {
            printf("FAIL ran without a device: status %d\n", a.status());
            return 1;
        }
        printf("OK nodevice\n");
        return 0;
    }
    if (PnPsolver::evaluate(all, scenes[0].calls.empty() ? 5 : scenes[0].calls[0]) != ORBX_OK || orbm_debug_last_pnp_waits() != 1) {
        printf("FAIL evaluate: %s\n", orbx_last_error());
        return 1;
    }
    printf("OK %d solvers in one call\n", (int)all.size());
    for (size_t k = 0; k < all.size(); ++k)
        for (int c : scenes[k].calls) {
            const bool found = all[k]->iterate(c, noMore, inl, nin, T);
            if (all[k]->status() != ORBX_OK) { printf("FAIL iterate: %s\n", orbx_last_error()); return 1; }
            printf("call %d %d %d %d", (int)k, (int)found, (int)noMore, nin);
            for (int q = 0; q < 16; ++q) {
                uint32_t w = 0;
                if (found) memcpy(&w, T + q, 4);
                printf(" %08x", w);
            }
            printf(" :");
            for (size_t i = 0; i < inl.size(); ++i) if (inl[i]) printf(" %d", (int)i);
            printf("\n");
        }
    return 0;
}
