// orbslam_hip::Sim3Solver (include/orbslam_hip.hpp) from C++, built and run by tests/test_cpu_sim3.py.  Two candidates whose pairs
// are exact under a known similarity (s = 1.7, 40 degrees about a skew axis, t != 0; the second with the scale fixed at 1), both
// poses the identity: one EvaluateBatch call evaluates both, every well-spread triple finds the similarity with all pairs as
// inliers, and iterate / find are folds without device work.  argv[1] = "nodevice": expect the first iterate to fail loudly.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using orbslam_hip::Sim3Solver;

static unsigned g_state = 12345u;
static int draw(int lo, int hi)      // a small LCG in place of DUtils::Random::RandomInt
{
    g_state = g_state * 1664525u + 1013904223u;
    return lo + (int)((g_state >> 8) % (unsigned)(hi - lo + 1));
}

static Sim3Solver::Problem make(int n, double s, bool fix, const double R[9], const double t[3])
{
    Sim3Solver::Problem p;
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(p.Tcw1, I, sizeof(I)); memcpy(p.Tcw2, I, sizeof(I));
    p.fx1 = p.fy1 = 500.f; p.cx1 = 320.f; p.cy1 = 240.f; p.fx2 = 480.f; p.fy2 = 490.f; p.cx2 = 315.f; p.cy2 = 236.f;
    for (int l = 0; l < 8; ++l) p.levelSigma2.push_back((float)std::pow(1.2, 2.0 * l));
    p.bFixScale = fix;
    p.N1 = 2 * n;
    for (int i = 0; i < n; ++i) {
        const double z = 2.0 + 6.0 * ((i * 37) % 101) / 101.0;
        const double x1[3] = {(((i * 53) % 97) / 97.0 - 0.5) * z, (((i * 29) % 89) / 89.0 - 0.5) * 0.8 * z, z};
        for (int r = 0; r < 3; ++r) {
            double v = 0;                                    // X2 = R^T (X1 - t) / s
            for (int k = 0; k < 3; ++k) v += R[3 * k + r] * (x1[k] - t[k]);
            p.X1w.push_back((float)x1[r]); p.X2w.push_back((float)(v / s));
        }
        p.octave1.push_back(i % 8); p.octave2.push_back((i + 3) % 8);
        p.indices1.push_back(2 * i);                         // the pairs stand at every second place of vpMatched12
    }
    return p;
}

int main(int argc, char **argv)
{
    const bool nodevice = argc > 1 && !strcmp(argv[1], "nodevice");
    const double ax[3] = {1 / std::sqrt(5.25), 2 / std::sqrt(5.25), -0.5 / std::sqrt(5.25)}, th = 40.0 * 3.14159265358979323846 / 180.0;
    double R[9];
    const double c = std::cos(th), sn = std::sin(th);
    const double K[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) R[3 * r + q] = (r == q ? c : 0.0) + (1 - c) * ax[r] * ax[q] + sn * K[3 * r + q];
    const double t[3] = {0.3, -0.2, 0.4};
    const int n = 70;
    Sim3Solver a(make(n, 1.7, false, R, t), &draw), b(make(n, 1.0, true, R, t), &draw);
    a.SetRansacParameters(0.99, 20, 300); b.SetRansacParameters(0.99, 20, 300);
    if (a.GetRansacMaxIts() < 50 || a.GetRansacMaxIts() > 300) { printf("FAIL mRansacMaxIts %d\n", a.GetRansacMaxIts()); return 1; }
    std::vector<bool> inl;
    int nin = -1;
    bool noMore = false;
    float T[16];
    if (nodevice) {
        const bool found = a.iterate(5, noMore, inl, nin, T);
        if (found || a.status() != ORBX_ERR_NO_DEVICE || !noMore || nin != 0 || (int)inl.size() != 2 * n) { printf("FAIL ran without a device: status %d\n", a.status()); return 1; }
        float Rb[9];
        if (a.GetEstimatedRotation(Rb)) { printf("FAIL an estimate without a device\n"); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    std::vector<Sim3Solver *> both;
    both.push_back(&a); both.push_back(&b);
    if (Sim3Solver::EvaluateBatch(both) != ORBX_OK || orbm_debug_last_sim3_waits() != 1) { printf("FAIL EvaluateBatch: %s\n", orbx_last_error()); return 1; }
    Sim3Solver *S[2] = {&a, &b};
    for (int k = 0; k < 2; ++k) {
        const double s = k ? 1.0 : 1.7;
        int rounds = 0, successes = 0;
        noMore = false;
        while (!noMore && rounds < S[k]->GetRansacMaxIts() + 2) {   // exact pairs: every call may succeed on its first iteration
            const bool found = S[k]->iterate(5, noMore, inl, nin, T);
            ++rounds;
            if (!found) continue;
            ++successes;
            float Rb[9], tb[3];
            if (!S[k]->GetEstimatedRotation(Rb) || !S[k]->GetEstimatedTranslation(tb)) { printf("FAIL no estimate\n"); return 1; }
            if (nin == n) {                                   // a triple that found the similarity: all pairs in, at their places
                double e = std::fabs(S[k]->GetEstimatedScale() - s);
                for (int q = 0; q < 9; ++q) e = std::max(e, std::fabs(Rb[q] - R[q]));
                for (int q = 0; q < 3; ++q) e = std::max(e, std::fabs(tb[q] - t[q]));
                for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) e = std::max(e, std::fabs(T[4 * r + q] - s * R[3 * r + q]));
                if (e > 1e-3) { printf("FAIL candidate %d: off by %g\n", k, e); return 1; }
                for (int i = 0; i < 2 * n; ++i) if (inl[i] != (i % 2 == 0)) { printf("FAIL candidate %d: inlier flag %d\n", k, i); return 1; }
            }
        }
        if (!noMore || successes < 1 || nin < 0) { printf("FAIL candidate %d: %d rounds %d successes\n", k, rounds, successes); return 1; }
    }
    if (orbm_debug_last_sim3_waits() != 1) { printf("FAIL device work after the first evaluation\n"); return 1; }
    printf("OK two candidates in one call\n");
    return 0;
}
