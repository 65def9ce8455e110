// One scene through orbslam_hip::EssentialGraph::OptimizeEnv (include/orbslam_hip.hpp) for
// tests/test_gpu_essential_graph_env.py::test_through_the_cxx_class.
//   essential_graph_env_smoke scene.bin out.bin iterations
// scene.bin: int32 nvert, ncorr, nnc, nedges, npoints, fix_scale; then poses [nvert][16] float, corrected [nvert] int32, corrected_sim3
// [ncorr][8] double, noncorrected [nvert] int32, noncorrected_sim3 [nnc][8] double, fixed [nvert] uint8, e_v0, e_v1 int32, e_kind uint8,
// points [npoints][3] float, p_ref int32.  out.bin: the poses, then the points.  The graph goes through the builder's calls.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbslam_hip.hpp"

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[6];
    if (fread(h, sizeof(int32_t), 6, f) != 6) return 2;
    const int nv = h[0], ncorr = h[1], nnc = h[2], ne = h[3], np = h[4];
    std::vector<float> poses, points;
    std::vector<int32_t> cor, nc, v0, v1, ref;
    std::vector<double> ctab, ntab;
    std::vector<uint8_t> fixed, kind;
    if (!rd(f, poses, 16 * (size_t)nv) || !rd(f, cor, nv) || !rd(f, ctab, 8 * (size_t)ncorr) || !rd(f, nc, nv) || !rd(f, ntab, 8 * (size_t)nnc) ||
        !rd(f, fixed, nv) || !rd(f, v0, ne) || !rd(f, v1, ne) || !rd(f, kind, ne) || !rd(f, points, 3 * (size_t)np) || !rd(f, ref, np))
        return 2;
    fclose(f);
    orbslam_hip::EssentialGraph eg;
    eg.fixScale = h[5] != 0;
    // (the builder numbers the table entries in keyframe order; a scene whose entries are numbered otherwise gives the same graph)
    for (int k = 0; k < nv; ++k)
        eg.addKeyFrame(&poses[16 * k], fixed[k] != 0, cor[k] >= 0 ? &ctab[8 * cor[k]] : nullptr, nc[k] >= 0 ? &ntab[8 * nc[k]] : nullptr);
    for (int e = 0; e < ne; ++e) {
        if (kind[e] == 0) eg.addLoopConnection(v0[e], v1[e]);
        else eg.addEdge(v0[e], v1[e]);
    }
    for (int n = 0; n < np; ++n) eg.addPoint(&points[3 * n], ref[n]);
    if (!eg.OptimizeEnv(atoi(argv[3]))) { printf("FAIL status %d: %s\n", eg.status(), orbx_last_error()); return 1; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(eg.poses.data(), sizeof(float), eg.poses.size(), o);
    fwrite(eg.points.data(), sizeof(float), eg.points.size(), o);
    fclose(o);
    printf("OK %d keyframes, %d edges, %d points\n", nv, ne, np);
    return 0;
}
