// orbslam_hip::Initializer (include/orbslam_hip.hpp) from C++, built and run by tests/test_gpu_init.py (and, without a device, by
// tests/test_cpu_init.py).  A 640 x 480 camera sees 120 points at depths 2 .. 8 from two poses, X2 = R X1 + t (6 degrees about a
// skew axis), exact up to float rounding, plus unmatched keypoints in both frames: Initialize draws its sets through the callback,
// finds both models in one launch, reconstructs from F and returns the motion.  argv[1] = "nodevice": expect a loud failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using orbslam_hip::Initializer;

static unsigned g_state = 12345u;
static int draw(int lo, int hi)      // a small LCG in place of DUtils::Random::RandomInt
{
    g_state = g_state * 1664525u + 1013904223u;
    return lo + (int)((g_state >> 8) % (unsigned)(hi - lo + 1));
}

int main(int argc, char **argv)
{
    const bool nodevice = argc > 1 && !strcmp(argv[1], "nodevice");
    const double ax[3] = {0.2 / std::sqrt(1.05), 1.0 / std::sqrt(1.05), -0.1 / std::sqrt(1.05)}, th = 6.0 * 3.14159265358979323846 / 180.0;
    const double c = std::cos(th), sn = std::sin(th);
    const double Kx[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) R[3 * r + q] = (r == q ? c : 0.0) + (1 - c) * ax[r] * ax[q] + sn * Kx[3 * r + q];
    const double t[3] = {1.0, 0.15, 0.1}, tn = std::sqrt(1.0 + 0.15 * 0.15 + 0.01);
    const float K[9] = {500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f};
    const int n = 120, extra = 7;
    std::vector<float> keys1, keys2;
    std::vector<int> matches12;
    for (int i = 0; i < extra; ++i) { keys2.push_back(30.f + 80.f * i); keys2.push_back(400.f - 45.f * i); }    // unmatched, in front of frame 2
    for (int i = 0; i < n; ++i) {
        const double u = 30.0 + 580.0 * ((i * 53) % 97) / 97.0, v = 30.0 + 420.0 * ((i * 29) % 89) / 89.0, z = 2.0 + 6.0 * ((i * 37) % 101) / 101.0;
        const double X[3] = {(u - 320.0) / 500.0 * z, (v - 240.0) / 500.0 * z, z};
        double Y[3];
        for (int r = 0; r < 3; ++r) Y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
        keys1.push_back((float)u); keys1.push_back((float)v);
        keys2.push_back((float)(500.0 * Y[0] / Y[2] + 320.0)); keys2.push_back((float)(500.0 * Y[1] / Y[2] + 240.0));
        matches12.push_back(extra + i);
    }
    for (int i = 0; i < extra; ++i) { keys1.push_back(50.f + 70.f * i); keys1.push_back(60.f + 50.f * i); matches12.push_back(-1); }   // unmatched, behind
    Initializer init(keys1, K, 1.0f, 200);
    float R21[9], t21[3];
    std::vector<float> P3D;
    std::vector<bool> tri;
    const Initializer::Status st = init.Initialize(keys2, matches12, &draw, R21, t21, P3D, tri);
    if (nodevice) {
        if (st != Initializer::FAILED || init.status() != ORBX_ERR_NO_DEVICE) { printf("FAIL ran without a device: %d status %d\n", (int)st, init.status()); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    if (st != Initializer::INITIALIZED) { printf("FAIL status %d (library %d: %s), RH %g\n", (int)st, init.status(), orbx_last_error(), init.RH()); return 1; }
    if (orbm_debug_last_init_waits() != 1) { printf("FAIL waits %d\n", orbm_debug_last_init_waits()); return 1; }
    double e = 0;
    for (int q = 0; q < 9; ++q) e = std::max(e, std::fabs(R21[q] - R[q]));
    for (int q = 0; q < 3; ++q) e = std::max(e, std::fabs(t21[q] - t[q] / tn));
    if (e > 1e-3) { printf("FAIL motion off by %g\n", e); return 1; }
    if ((int)init.matches12().size() != 2 * n || (int)init.sets().size() != 8 * 200 || (int)tri.size() != n + extra) { printf("FAIL sizes\n"); return 1; }
    const std::vector<bool> inF = init.inliersF();
    for (int i = 0; i < n; ++i) {
        if (!inF[i] || !tri[i]) { printf("FAIL match %d: inlier %d triangulated %d\n", i, (int)inF[i], (int)tri[i]); return 1; }
        const double z = 2.0 + 6.0 * ((i * 37) % 101) / 101.0;
        if (std::fabs(P3D[3 * i + 2] * tn - z) > 2e-2) { printf("FAIL depth of %d: %g against %g\n", i, P3D[3 * i + 2] * tn, z); return 1; }
    }
    for (int i = n; i < n + extra; ++i) if (tri[i] || P3D[3 * i + 2] != 0.0f) { printf("FAIL unmatched keypoint %d written\n", i); return 1; }
    if (!(init.RH() < 0.99f) || init.models().itF < 0 || init.reconstruction().N != n) { printf("FAIL RH %g itF %d N %d\n", init.RH(), init.models().itF, init.reconstruction().N); return 1; }
    printf("OK initialised: RH %.3f, %d triangulated, parallax %.2f\n", init.RH(), init.reconstruction().max_good, init.reconstruction().parallax[init.reconstruction().best]);
    return 0;
}
