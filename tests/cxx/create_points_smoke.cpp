// LocalMapping::CreateNewMapPoints as one call from C++ (include/orbslam_hip.hpp: ORBmatcher::CreateNewMapPoints), built and run by
// tests/test_cxx_create_points.py.  A current keyframe at the origin and two neighbours shifted sideways see N points exactly;
// every keypoint has a vocabulary node of its own and the neighbours hold the keypoints in reverse order.  Keypoint 0 of
// neighbour 0 sits at the current keyframe's pixel (identical rays: a parallax reject), so: N - 1 points against neighbour 0 in
// index order, keypoint 0 against neighbour 1, the other rows skipped.  argv[1] = "nodevice": expect the call to fail loudly.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

int main(int argc, char **argv)
{
    const bool nodevice = argc > 1 && !strcmp(argv[1], "nodevice");
    const int N = 40;
    const float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f;
    const double C[2][3] = {{0.5, 0.0, 0.05}, {-0.4, 0.1, -0.05}};      // the neighbours' centres; no rotation anywhere
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::vector<float> X(3 * N), sf, sg;
    for (int l = 0; l < 8; ++l) { sf.push_back(std::pow(1.2f, (float)l)); sg.push_back(sf[l] * sf[l]); }
    std::vector<orbx_keypoint> kps[3];
    std::vector<uint8_t> desc[3], has[3];
    ORBmatcher::FeatureVector fv[3];
    for (int f = 0; f < 3; ++f) { kps[f].resize(N); desc[f].resize(32 * N); has[f].assign(N, 0); }
    for (int i = 0; i < N; ++i) {
        const float z = 3.f + 3.f * U(rng);
        X[3 * i] = (U(rng) - 0.5f) * 0.8f * z; X[3 * i + 1] = (U(rng) - 0.5f) * 0.6f * z; X[3 * i + 2] = z;
        for (int b = 0; b < 32; ++b) desc[0][32 * i + b] = (uint8_t)(rng() & 0xff);
    }
    std::vector<int32_t> node[3];
    for (int f = 0; f < 3; ++f) {
        node[f].resize(N);
        for (int i = 0; i < N; ++i) {
            const int j = f == 0 ? i : N - 1 - i;                        // where point i stands in this frame
            const double c0 = f ? C[f - 1][0] : 0.0, c1 = f ? C[f - 1][1] : 0.0, c2 = f ? C[f - 1][2] : 0.0;
            memset(&kps[f][j], 0, sizeof(orbx_keypoint));
            kps[f][j].x = (float)(fx * (X[3 * i] - c0) / (X[3 * i + 2] - c2) + cx);
            kps[f][j].y = (float)(fy * (X[3 * i + 1] - c1) / (X[3 * i + 2] - c2) + cy);
            kps[f][j].octave = 2;
            memcpy(&desc[f][32 * j], &desc[0][32 * i], 32);
            node[f][j] = 10 + 2 * i;
        }
        fv[f] = ORBmatcher::FeatureVector::FromNodeIds(node[f]);
    }
    kps[1][N - 1].x = kps[0][0].x; kps[1][N - 1].y = kps[0][0].y;     // point 0 in neighbour 0: the same pixel
    float T[3][16];
    ORBmatcher::FrameView V[3];
    for (int f = 0; f < 3; ++f) {
        const float t[16] = {1, 0, 0, f ? (float)-C[f - 1][0] : 0.f, 0, 1, 0, f ? (float)-C[f - 1][1] : 0.f, 0, 0, 1, f ? (float)-C[f - 1][2] : 0.f, 0, 0, 0, 1};
        memcpy(T[f], t, sizeof(t));
        V[f].mvKeysUn = kps[f].data(); V[f].mDescriptors = desc[f].data(); V[f].N = N; V[f].mnMinX = 0; V[f].mnMinY = 0; V[f].mnMaxX = 640; V[f].mnMaxY = 480;
    }
    ORBmatcher::ResidentFrame R0(V[0]), R1(V[1]), R2(V[2]);
    const ORBmatcher::ResidentFrame *R[3] = {&R0, &R1, &R2};
    auto kf = [&](int f) {
        ORBmatcher::TriangKeyFrame k;
        k.frame = R[f]; k.Tcw = T[f]; k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.invfx = 1.f / fx; k.invfy = 1.f / fy; k.mb = 0.2f; k.mbf = 100.f;
        k.depth = nullptr; k.hasMP = &has[f]; k.fv = &fv[f];
        return k;
    };
    std::vector<ORBmatcher::Neighbour> nb(2);
    for (int f = 1; f < 3; ++f) {
        // F12 = K^-T [t12]x K^-1 with t12 = the neighbour's centre; the epipole = the current centre seen from the neighbour
        const double *c = C[f - 1];
        const double tx[9] = {0, -c[2], c[1], c[2], 0, -c[0], -c[1], c[0], 0};
        const double Ki[9] = {1.0 / fx, 0, -cx / (double)fx, 0, 1.0 / fy, -cy / (double)fy, 0, 0, 1};
        double M[9], F[9];
        for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { M[3 * r + q] = 0; for (int s = 0; s < 3; ++s) M[3 * r + q] += tx[3 * r + s] * Ki[3 * s + q]; }
        for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { F[3 * r + q] = 0; for (int s = 0; s < 3; ++s) F[3 * r + q] += Ki[3 * s + r] * M[3 * s + q]; }
        nb[f - 1].kf = kf(f);
        for (int q = 0; q < 9; ++q) nb[f - 1].F12[q] = (float)F[q];
        nb[f - 1].ex = (float)(fx * (-c[0]) / (-c[2]) + cx); nb[f - 1].ey = (float)(fy * (-c[1]) / (-c[2]) + cy);
    }
    ORBmatcher m(0.6f, false);
    std::vector<ORBmatcher::NewPoint> made;
    ORBmatcher::NewPointCounters cnt;
    if (nodevice) {
        const int n = m.CreateNewMapPoints(kf(0), sf, sg, 1.2f, nb, made, cnt);
        if (m.status() == ORBX_OK || n != 0 || !made.empty()) { printf("FAIL CreateNewMapPoints ran without a device\n"); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    for (int f = 0; f < 3; ++f) if (R[f]->status() != ORBX_OK) { printf("FAIL frame %d\n", R[f]->status()); return 1; }
    const int n = m.CreateNewMapPoints(kf(0), sf, sg, 1.2f, nb, made, cnt);
    if (m.status() != ORBX_OK || n != N || cnt.nnew != N || (int)made.size() != N || orbm_debug_last_create_points_waits() != 1) {
        printf("FAIL status %d nnew %d / %d list %d waits %d\n", m.status(), n, cnt.nnew, (int)made.size(), orbm_debug_last_create_points_waits());
        return 1;
    }
    if (cnt.nParalaxRejects != 1 || cnt.nTriangulationRejects || cnt.nDepthRejects || cnt.nRepErrorRejects || cnt.nScaleConsRejects) {
        printf("FAIL counters %d %d %d %d %d\n", cnt.nTriangulationRejects, cnt.nParalaxRejects, cnt.nDepthRejects, cnt.nRepErrorRejects, cnt.nScaleConsRejects);
        return 1;
    }
    for (int e = 0; e < N; ++e) {      // (k, idx1) ascending: keypoints 1 .. N-1 against neighbour 0, then keypoint 0 against neighbour 1
        const ORBmatcher::NewPoint &p = made[e];
        const int i = e < N - 1 ? e + 1 : 0, k = e < N - 1 ? 0 : 1;
        double d = 0;
        for (int q = 0; q < 3; ++q) d = std::max(d, (double)std::fabs(p.x3D[q] - X[3 * i + q]));
        if (p.k != k || p.idx1 != i || p.idx2 != N - 1 - i || d > 1e-3) { printf("FAIL entry %d: k %d idx1 %d idx2 %d off by %g\n", e, p.k, p.idx1, p.idx2, d); return 1; }
    }
    // no neighbours: nothing to do
    const int n0 = m.CreateNewMapPoints(kf(0), sf, sg, 1.2f, std::vector<ORBmatcher::Neighbour>(), made, cnt);
    if (m.status() != ORBX_OK || n0 != 0 || !made.empty() || cnt.nnew != 0 || orbm_debug_last_create_points_waits() != 0) { printf("FAIL K = 0\n"); return 1; }
    printf("OK %d points, 1 parallax reject\n", N);
    return 0;
}
