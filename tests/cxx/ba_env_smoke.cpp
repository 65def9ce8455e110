// One scene through orbslam_hip::BundleAdjustment (include/orbslam_hip.hpp) for tests/test_gpu_ba_env.py::test_through_the_cxx_class.
//   ba_env_smoke scene.bin out.bin
// scene.bin: int32 nfree, nfixed, npoints, nedges; then poses [nfree + nfixed][16] float, fixed [nfree] uint8, points [npoints][3]
// float, e_point, e_cam int32, e_obs [ne][3], e_inv_sigma2 [ne], e_cam_k [ne][5] float.  out.bin: int32 stopped, the poses of the
// free keyframes, the points, notIncluded.  The graph goes through the builder's calls; GlobalMapEnv(10, false) runs: the global BA behind a
// loop closure of a long session, over orbm_global_bundle_adjustment_env (the keyframes of the file are in ascending mnId).
#include <cstdio>
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
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[4];
    if (fread(h, sizeof(int32_t), 4, f) != 4) return 2;
    const int nfree = h[0], nfixed = h[1], npoints = h[2], ne = h[3];
    std::vector<float> poses, points, obs, info, K;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ep, ec;
    if (!rd(f, poses, 16 * (size_t)(nfree + nfixed)) || !rd(f, fixed, nfree) || !rd(f, points, 3 * (size_t)npoints) || !rd(f, ep, ne) || !rd(f, ec, ne) ||
        !rd(f, obs, 3 * (size_t)ne) || !rd(f, info, ne) || !rd(f, K, 5 * (size_t)ne))
        return 2;
    fclose(f);
    orbslam_hip::BundleAdjustment ba;
    for (int k = 0; k < nfree; ++k) ba.addKeyFrame(&poses[16 * k], fixed[k] != 0);
    for (int k = 0; k < nfixed; ++k) ba.addFixedKeyFrame(&poses[16 * (nfree + k)]);
    for (int n = 0, e = 0; n < npoints; ++n) {
        ba.addPoint(&points[3 * n]);
        for (; e < ne && ep[e] == n; ++e) ba.addObservation(ec[e], obs[3 * e], obs[3 * e + 1], obs[3 * e + 2], info[e], K[5 * e], K[5 * e + 1], K[5 * e + 2], K[5 * e + 3], K[5 * e + 4]);
    }
    if (!ba.GlobalMapEnv(10, false)) { printf("FAIL status %d: %s\n", ba.status(), orbx_last_error()); return 1; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t stopped = ba.stopped;
    fwrite(&stopped, sizeof(stopped), 1, o);
    fwrite(ba.poses.data(), sizeof(float), 16 * (size_t)nfree, o);
    fwrite(ba.points.data(), sizeof(float), ba.points.size(), o);
    fwrite(ba.notIncluded.data(), 1, ba.notIncluded.size(), o);
    fclose(o);
    printf("OK %d keyframes, %d points, %d edges\n", nfree + nfixed, npoints, ne);
    return 0;
}
