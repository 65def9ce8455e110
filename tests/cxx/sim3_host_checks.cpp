// The host side of orbm_sim3_hypotheses as a stand-alone program for tools/sim3_sanitize.sh (AddressSanitizer +
// UndefinedBehaviorSanitizer on the host code, run on the CPU): every refusal that comes before the launch, the calls that launch
// nothing, and, on a machine without a device, the loud failure of a valid call.  Exit status 0 = every answer as expected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                                     \
    do {                                                                                       \
        const int got__ = (call);                                                              \
        if (got__ != (want)) { printf("FAIL line %d: %d, expected %d (%s)\n", __LINE__, got__, (want), orbx_last_error()); ++failures; } \
    } while (0)

struct Case {
    std::vector<float> X1, X2, sigma2;
    std::vector<int32_t> o1, o2, tri;
    float T[16];
    orbm_sim3_problem p;
    Case(int n, int H) : X1(3 * (n > 0 ? n : 1)), X2(3 * (n > 0 ? n : 1)), sigma2(8, 1.44f), o1(n > 0 ? n : 1, 2), o2(n > 0 ? n : 1, 7), tri(3 * (H > 0 ? H : 1))
    {
        for (int i = 0; i < 3 * n; ++i) { X1[i] = 1.f + 0.37f * (float)((i * 7) % 11); X2[i] = 2.f + 0.21f * (float)((i * 5) % 13); }
        for (int h = 0; h < H; ++h) { tri[3 * h] = h % n; tri[3 * h + 1] = (h + 1) % n; tri[3 * h + 2] = (h + 2) % n; }
        const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        memcpy(T, I, sizeof(I));
        refresh(n, H);
    }
    void refresh(int n, int H)
    {
        p.X1w = X1.data(); p.X2w = X2.data(); p.octave1 = o1.data(); p.octave2 = o2.data(); p.Tcw1 = T; p.Tcw2 = T;
        p.fx1 = p.fy1 = p.fx2 = p.fy2 = 500.f; p.cx1 = p.cx2 = 320.f; p.cy1 = p.cy2 = 240.f;
        p.triples = tri.data(); p.n = n; p.H = H; p.fix_scale = 0;
    }
};

int main()
{
    std::vector<orbm_sim3_hypothesis> hyp(4096);
    std::vector<uint64_t> masks(1 << 16);
    Case good(100, 30);
    const float *sg = good.sigma2.data();
    // nothing to do
    EXPECT(orbm_sim3_hypotheses(nullptr, 0, sg, 8, hyp.data(), masks.data()), ORBX_OK);
    EXPECT(orbm_sim3_hypotheses(nullptr, 0, nullptr, 0, nullptr, nullptr), ORBX_OK);
    { Case a(100, 0), b(2, 0); orbm_sim3_problem two[2] = {a.p, b.p}; EXPECT(orbm_sim3_hypotheses(two, 2, sg, 8, hyp.data(), masks.data()), ORBX_OK); }
    EXPECT(orbm_debug_last_sim3_waits(), 0);
    // limits
    { std::vector<orbm_sim3_problem> many(65, good.p); EXPECT(orbm_sim3_hypotheses(many.data(), 65, sg, 8, hyp.data(), masks.data()), ORBX_ERR_UNSUPPORTED); }
    { Case c(8193, 1); EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_UNSUPPORTED); }
    { Case c(10, 1025); EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_UNSUPPORTED); }
    // argument errors
    EXPECT(orbm_sim3_hypotheses(&good.p, -1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG);
    EXPECT(orbm_sim3_hypotheses(nullptr, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG);
    EXPECT(orbm_sim3_hypotheses(&good.p, 1, nullptr, 8, hyp.data(), masks.data()), ORBX_ERR_ARG);
    EXPECT(orbm_sim3_hypotheses(&good.p, 1, sg, 0, hyp.data(), masks.data()), ORBX_ERR_ARG);
    EXPECT(orbm_sim3_hypotheses(&good.p, 1, sg, 8, nullptr, masks.data()), ORBX_ERR_ARG);
    EXPECT(orbm_sim3_hypotheses(&good.p, 1, sg, 8, hyp.data(), nullptr), ORBX_ERR_ARG);
    { Case c(2, 0); c.tri[0] = 0; c.tri[1] = 1; c.tri[2] = 0; c.refresh(2, 1); EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.tri[5] = 10; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.tri[9] = -1; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.tri[3] = c.tri[5]; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.o1[9] = 8; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.o2[0] = -1; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); c.p.n = -1; EXPECT(orbm_sim3_hypotheses(&c.p, 1, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    { Case c(10, 4); orbm_sim3_problem three[3] = {good.p, good.p, c.p}; three[2].X2w = nullptr; EXPECT(orbm_sim3_hypotheses(three, 3, sg, 8, hyp.data(), masks.data()), ORBX_ERR_ARG); }
    EXPECT(orbm_debug_last_sim3_waits(), 0);
    // a valid call: needs a device
    const int rc = orbm_sim3_hypotheses(&good.p, 1, sg, 8, hyp.data(), masks.data());
    if (rc == ORBX_ERR_NO_DEVICE) EXPECT(orbm_debug_last_sim3_waits(), 0);
    else if (rc == ORBX_OK) EXPECT(orbm_debug_last_sim3_waits(), 1);
    else { printf("FAIL valid call: %d (%s)\n", rc, orbx_last_error()); ++failures; }
    printf(failures ? "FAILED %d\n" : "OK sim3 host checks (valid call: %d)\n", failures ? failures : rc);
    return failures ? 1 : 0;
}
