// orbslam_hip::OptimizeSim3 (include/orbslam_hip.hpp) from C++, built and run by tests/test_cpu_sim3_opt.py.  Two problems whose
// observations are the exact projections of points related by a known similarity (s = 1.7, 40 degrees about a skew axis, t != 0;
// the second with the scale fixed at 1), three of the 60 pairs of each moved 40 px away, both poses the identity, the start 3
// degrees / 3 % off: one call refines both, cuts exactly the moved pairs and lands on the similarity.  argv[1] = "nodevice": expect
// ORBX_ERR_NO_DEVICE, loudly.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using orbslam_hip::Sim3OptProblem;

static void rodrigues(const double ax[3], double deg, double R[9])
{
    const double th = deg * 3.14159265358979323846 / 180.0, c = std::cos(th), sn = std::sin(th);
    const double K[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) R[3 * r + q] = (r == q ? c : 0.0) + (1 - c) * ax[r] * ax[q] + sn * K[3 * r + q];
}

static Sim3OptProblem make(int n, double s, bool fix, const double R[9], const double t[3])
{
    Sim3OptProblem p;
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    memcpy(p.Tcw1, I, sizeof(I)); memcpy(p.Tcw2, I, sizeof(I));
    p.fx1 = p.fy1 = 500.f; p.cx1 = 320.f; p.cy1 = 240.f; p.fx2 = 480.f; p.fy2 = 490.f; p.cx2 = 315.f; p.cy2 = 236.f;
    p.bFixScale = fix;
    p.th2 = 10.f;
    for (int i = 0; i < n; ++i) {
        const double z = 2.0 + 6.0 * ((i * 37) % 101) / 101.0;
        const double x1[3] = {(((i * 53) % 97) / 97.0 - 0.5) * z, (((i * 29) % 89) / 89.0 - 0.5) * 0.8 * z, z};
        double x2[3];
        for (int r = 0; r < 3; ++r) {
            double v = 0;                                    // X2 = R^T (X1 - t) / s
            for (int k = 0; k < 3; ++k) v += R[3 * k + r] * (x1[k] - t[k]);
            x2[r] = v / s;
            p.X1w.push_back((float)x1[r]); p.X2w.push_back((float)x2[r]);
        }
        // the observations of the float points, so that the similarity is exact for what the library is given
        const float a[3] = {p.X1w[3 * i], p.X1w[3 * i + 1], p.X1w[3 * i + 2]}, b[3] = {p.X2w[3 * i], p.X2w[3 * i + 1], p.X2w[3 * i + 2]};
        p.obs1.push_back((float)(500.0 * a[0] / a[2] + 320.0)); p.obs1.push_back((float)(500.0 * a[1] / a[2] + 240.0));
        p.obs2.push_back((float)(480.0 * b[0] / b[2] + 315.0) + (i % 20 == 7 ? 40.f : 0.f)); p.obs2.push_back((float)(490.0 * b[1] / b[2] + 236.0));
        p.octave1.push_back(i % 8); p.octave2.push_back((i + 3) % 8);
    }
    const double off_axis[3] = {0.6, 0.0, 0.8};
    double Roff[9];
    rodrigues(off_axis, 3.0, Roff);
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) {
            double v = 0;
            for (int k = 0; k < 3; ++k) v += R[3 * r + k] * Roff[3 * k + q];
            p.R12[3 * r + q] = (float)v;
        }
        p.t12[r] = (float)(1.03 * t[r]);
    }
    p.s12 = (float)(fix ? 1.0 : 1.03 * s);
    return p;
}

int main(int argc, char **argv)
{
    const bool nodevice = argc > 1 && !strcmp(argv[1], "nodevice");
    const double ax[3] = {1 / std::sqrt(5.25), 2 / std::sqrt(5.25), -0.5 / std::sqrt(5.25)};
    double R[9];
    rodrigues(ax, 40.0, R);
    const double t[3] = {0.3, -0.2, 0.4};
    const int n = 60;
    std::vector<Sim3OptProblem> probs;
    probs.push_back(make(n, 1.7, false, R, t)); probs.push_back(make(n, 1.0, true, R, t));
    std::vector<float> inv;
    for (int l = 0; l < 8; ++l) inv.push_back(1.0f / (float)std::pow(1.2, 2.0 * l));
    std::vector<orbm_sim3_opt_result> res;
    std::vector<std::vector<uint8_t> > kept;
    const int rc = orbslam_hip::OptimizeSim3(probs, inv, res, kept);
    if (nodevice) {
        if (rc != ORBX_ERR_NO_DEVICE || orbm_debug_last_sim3_opt_waits() != 0) { printf("FAIL ran without a device: rc %d\n", rc); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    if (rc != ORBX_OK || orbm_debug_last_sim3_opt_waits() != 1) { printf("FAIL OptimizeSim3: %s\n", orbx_last_error()); return 1; }
    for (int k = 0; k < 2; ++k) {
        const double s = k ? 1.0 : 1.7;
        const orbm_sim3_opt_result &r = res[k];
        if (r.ncorrespondences != n || r.nbad != 3 || r.nin != n - 3) { printf("FAIL problem %d: nin %d nbad %d\n", k, r.nin, r.nbad); return 1; }
        for (int i = 0; i < n; ++i)
            if (kept[k][i] != (i % 20 == 7 ? 0 : 1)) { printf("FAIL problem %d: kept[%d]\n", k, i); return 1; }
        // the rotation of the quaternion (x y z w; not normalised by g2o) against R
        const double nq = std::sqrt(r.q[0] * r.q[0] + r.q[1] * r.q[1] + r.q[2] * r.q[2] + r.q[3] * r.q[3]);
        const double x = r.q[0] / nq, y = r.q[1] / nq, z = r.q[2] / nq, w = r.q[3] / nq;
        const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                              2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        double e = std::fabs(r.s - s);
        for (int q = 0; q < 9; ++q) e = std::max(e, std::fabs(Rq[q] - R[q]));
        for (int q = 0; q < 3; ++q) e = std::max(e, std::fabs(r.t[q] - t[q]));
        if (!(e < 1e-4)) { printf("FAIL problem %d: off by %g\n", k, e); return 1; }
        if (k == 1 && r.s != 1.0) { printf("FAIL the fixed scale moved\n"); return 1; }
    }
    printf("OK two problems in one call\n");
    return 0;
}
