// orbslam_hip::PoseOptimizationNR (include/orbslam_hip.hpp): Compute() and one call of the device bundle on a flat graph.  Built and
// run by tests/test_gpu_pose_nr.py, which compares what it writes with the Python binding's call on the same scene, byte for byte.
// usage: pose_nr_device_smoke <scene.bin> <out.bin>
//   scene: int32 {nElType, nTop, nFaces, nVertices, nDerived, nKF, nEdges}, f32 top[3 nTop], i32 faces[nv nFaces], i32 derived[4 nDerived],
//          f32 Tcw[16], kfTcw[16 nKF], points[3 nVertices], i32 e_point[nEdges], e_cam[nEdges], f32 e_obs[2 nEdges], e_inv_sigma2[nEdges],
//          e_cam_k[4 nEdges]
//   out:   int32 ngood, nTrials, nResults; f32 Tcw[16], points[3 nVertices]; u8 outlier[nVertices]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

template <class T> static void rd(FILE *f, T *v, size_t n)
{
    if (n && fread(v, sizeof(T), n, f) != n) { fprintf(stderr, "short scene\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[7]; rd(f, hd, 7);
    const int nElType = hd[0], nTop = hd[1], nFaces = hd[2], nVertices = hd[3], nDerived = hd[4], nKF = hd[5], nEdges = hd[6];
    std::vector<float> top((size_t)3 * nTop); rd(f, top.data(), top.size());
    std::vector<int32_t> faces((size_t)(nElType == 1 ? 4 : 3) * nFaces); rd(f, faces.data(), faces.size());
    std::vector<int32_t> derived((size_t)4 * nDerived); rd(f, derived.data(), derived.size());
    float Tcw[16]; rd(f, Tcw, 16);
    PoseOptimizationNR::Graph g;
    g.kfTcw.resize((size_t)16 * nKF); rd(f, g.kfTcw.data(), g.kfTcw.size());
    std::vector<float> points((size_t)3 * nVertices); rd(f, points.data(), points.size());
    g.ePoint.resize(nEdges); rd(f, g.ePoint.data(), g.ePoint.size());
    g.eCam.resize(nEdges); rd(f, g.eCam.data(), g.eCam.size());
    g.eObs.resize((size_t)2 * nEdges); rd(f, g.eObs.data(), g.eObs.size());
    g.eInvSigma2.resize(nEdges); rd(f, g.eInvSigma2.data(), g.eInvSigma2.size());
    g.eCamK.resize((size_t)4 * nEdges); rd(f, g.eCamK.data(), g.eCamK.size());
    fclose(f);

    PoseOptimizationNR nr(nElType);
    if (!nr.Compute(top, faces, nVertices, derived)) { fprintf(stderr, "Compute(1) failed: %d %s\n", nr.status(), orbx_last_error()); return 1; }
    std::vector<uint8_t> outlier;
    orbm_pose_nr_stats st = {};
    const int ngood = nr(g, Tcw, points, outlier, &st);
    if (ngood < 0) { fprintf(stderr, "status %d %s\n", nr.status(), orbx_last_error()); return 1; }
    // a graph that breaks the grouping is refused with the library's code and leaves the pose as it is
    if (nEdges >= 2 && g.ePoint[0] != g.ePoint[nEdges - 1]) {
        PoseOptimizationNR::Graph bad = g;
        std::swap(bad.ePoint[0], bad.ePoint[nEdges - 1]);
        float T2[16];
        for (int i = 0; i < 16; ++i) T2[i] = Tcw[i];
        std::vector<float> p2 = points;
        std::vector<uint8_t> o2;
        if (nr(bad, T2, p2, o2) != -1 || nr.status() != ORBX_ERR_ARG) { fprintf(stderr, "an ungrouped graph was not refused\n"); return 1; }
        for (int i = 0; i < 16; ++i) if (T2[i] != Tcw[i]) { fprintf(stderr, "a refused call changed the pose\n"); return 1; }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t cnt[3] = {ngood, st.ntrials, st.nresults};
    fwrite(cnt, 4, 3, o);
    fwrite(Tcw, 4, 16, o); fwrite(points.data(), 4, points.size(), o); fwrite(outlier.data(), 1, outlier.size(), o);
    fclose(o);
    printf("OK %d inliers, %d trials, %d iterations\n", ngood, (int)st.ntrials, (int)st.nresults);
    return 0;
}
