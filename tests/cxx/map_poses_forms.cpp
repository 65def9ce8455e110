// orbslam_hip::ORBmatcher::SearchByProjection over a MapSnapshot and several poses from C++ (include/orbslam_hip.hpp), built and
// run by tests/test_gpu_map_poses.py / tests/test_cpu_map_poses.py.  argv[1] = a scene written by the test (ints n, m, P, nlevels;
// float th; orbm_camera; then kps, desc, has, pos, normal, min, max, map descriptors, Rcw, tcw, scale factors), argv[2] = where
// the rows go: matched[P][n] and nmatches[P] of the ResidentFrame form, then the same of the FrameView form.
// argv[1] = "nodevice": the snapshot and the search must fail loudly.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n + 1); return fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "nodevice")) {
        const float z[3] = {0.f, 0.f, 1.f};
        const uint8_t d[32] = {0};
        ORBmatcher::MapSnapshot snap(z, z, z, z, d, 1);
        if (snap.status() != ORBX_ERR_NO_DEVICE || snap.handle()) { printf("FAIL snapshot status %d\n", snap.status()); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4]; float th; orbm_camera cam;
    if (fread(hdr, 4, 4, f) != 4 || fread(&th, 4, 1, f) != 1 || fread(&cam, sizeof(cam), 1, f) != 1) return 2;
    const int n = hdr[0], m = hdr[1], P = hdr[2], nl = hdr[3];
    std::vector<orbx_keypoint> kps; std::vector<uint8_t> desc, has, md; std::vector<float> pos, nrm, mn, mx, sf; std::vector<double> R, t;
    if (!rd(f, kps, n) || !rd(f, desc, 32 * (size_t)n) || !rd(f, has, n) || !rd(f, pos, 3 * (size_t)m) || !rd(f, nrm, 3 * (size_t)m) ||
        !rd(f, mn, m) || !rd(f, mx, m) || !rd(f, md, 32 * (size_t)m) || !rd(f, R, 9 * (size_t)P) || !rd(f, t, 3 * (size_t)P) || !rd(f, sf, nl))
        return 2;
    fclose(f);
    has.resize(n); sf.resize(nl);
    ORBmatcher::FrameView V;
    V.mvKeysUn = kps.data(); V.mDescriptors = desc.data(); V.N = n;
    V.mnMinX = cam.grid_min_x; V.mnMinY = cam.grid_min_y; V.mnMaxX = cam.grid_max_x; V.mnMaxY = cam.grid_max_y;
    ORBmatcher::ResidentFrame F(V);
    ORBmatcher::MapSnapshot snap(pos.data(), nrm.data(), mn.data(), mx.data(), md.data(), m);
    if (F.status() != ORBX_OK || snap.status() != ORBX_OK || snap.N != m) { printf("FAIL handles %d %d\n", F.status(), snap.status()); return 1; }
    std::vector<ORBmatcher::MapPose> poses(P);
    for (int p = 0; p < P; ++p) { memcpy(poses[p].Rcw, &R[9 * p], sizeof(double) * 9); memcpy(poses[p].tcw, &t[3 * p], sizeof(double) * 3); }
    ORBmatcher matcher(0.6f, true);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int form = 0; form < 2; ++form) {
        std::vector<std::vector<int32_t>> rows; std::vector<int> nm;
        const bool ok = form == 0 ? matcher.SearchByProjection(F, has, snap, poses, cam, sf, th, rows, nm)
                                  : matcher.SearchByProjection(V, has, snap, poses, cam, sf, th, rows, nm);
        if (!ok || (int)rows.size() != P || (int)nm.size() != P) { printf("FAIL form %d status %d\n", form, matcher.status()); return 1; }
        for (int p = 0; p < P; ++p) fwrite(rows[p].data(), sizeof(int32_t), n, o);
        for (int p = 0; p < P; ++p) { const int32_t v = nm[p]; fwrite(&v, sizeof(v), 1, o); }
    }
    fclose(o);
    printf("OK %d poses\n", P);
    return 0;
}
