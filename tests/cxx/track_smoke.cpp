// The tracking functions as one call from C++ (include/orbslam_hip.hpp: ORBmatcher::TrackWithMotionModel / TrackLocalMap), built
// and run by tests/test_cxx_track.py.  A small synthetic scene: points in front of a camera at the origin, one keypoint per
// point.  Each one-call result must equal the search followed by PoseOptimization over the gathered matches, bit for bit.
// argv[1] = "nodevice": expect ORBX_ERR_NO_DEVICE.
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
    const int N = 600;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    ORBmatcher::Calibration K;
    K.fx = 517.3f; K.fy = 516.5f; K.cx = 318.6f; K.cy = 255.3f; K.mbf = 40.f; K.mb = K.mbf / K.fx; K.mfLogScaleFactor = std::log(1.2f);
    std::vector<float> inv;
    for (int l = 0; l < 8; ++l) { K.mvScaleFactors.push_back(std::pow(1.2f, (float)l)); inv.push_back(1.f / (K.mvScaleFactors[l] * K.mvScaleFactors[l])); }
    std::vector<orbx_keypoint> kps(N);
    std::vector<uint8_t> desc(32 * N);
    std::vector<float> uright(N);
    ORBmatcher::PointList last;
    last.resize(N, false, false, true);
    for (int i = 0; i < N; ++i) {
        const float z = 2.f + 8.f * U(rng), x = (U(rng) - 0.5f) * z, y = (U(rng) - 0.5f) * 0.8f * z;
        memset(&kps[i], 0, sizeof(kps[i]));
        kps[i].x = K.fx * x / z + K.cx + (U(rng) - 0.5f); kps[i].y = K.fy * y / z + K.cy + (U(rng) - 0.5f);
        kps[i].octave = (int)(U(rng) * 3.f); kps[i].angle = 360.f * U(rng);
        uright[i] = (i % 3) ? kps[i].x - K.mbf / z : -1.f;
        for (int b = 0; b < 32; ++b) desc[32 * i + b] = (uint8_t)(rng() & 0xff);
        last.valid[i] = (i % 10) != 0; last.takes[i] = (i % 4) != 0; last.octave[i] = kps[i].octave; last.angle[i] = kps[i].angle;
        last.pos[3 * i] = x; last.pos[3 * i + 1] = y; last.pos[3 * i + 2] = z;
        memcpy(&last.desc[32 * i], &desc[32 * i], 32);
        last.desc[32 * i] ^= 1;
    }
    float T[16] = {1, 0, 0, 0.01f, 0, 1, 0, -0.01f, 0, 0, 1, 0.02f, 0, 0, 0, 1};   // the predicted pose: a little off
    ORBmatcher::FrameView F;
    F.mvKeysUn = kps.data(); F.mDescriptors = desc.data(); F.N = N; F.mvuRight = uright.data(); F.mnMinX = 0; F.mnMinY = 0; F.mnMaxX = 640; F.mnMaxY = 480;
    ORBmatcher::ResidentFrame cur(F);
    ORBmatcher m(0.9f, true);
    std::vector<int32_t> owner, owner2;
    std::vector<uint8_t> out, out2;
    float Tout[16];
    if (nodevice) {
        if (cur.status() != ORBX_ERR_NO_DEVICE) { printf("FAIL frame: expected ORBX_ERR_NO_DEVICE, got %d\n", cur.status()); return 1; }
        m.TrackWithMotionModel(cur, K, inv, T, T, last, 7.f, false, owner, out, Tout);
        if (m.status() == ORBX_OK) { printf("FAIL TrackWithMotionModel ran without a device\n"); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    if (cur.status() != ORBX_OK) { printf("FAIL frame %d\n", cur.status()); return 1; }

    // TrackWithMotionModel against SearchByProjection(Cur, Last) + PoseOptimization
    const orbm_track_result r = m.TrackWithMotionModel(cur, K, inv, T, T, last, 7.f, false, owner, out, Tout);
    if (m.status() != ORBX_OK || !r.tracked || r.search_used != 1 || r.nsearch < 100 || r.ngood < 50) {
        printf("FAIL TrackWithMotionModel status %d tracked %d search %d nsearch %d ngood %d\n", m.status(), r.tracked, r.search_used, r.nsearch, r.ngood);
        return 1;
    }
    const int nm = m.SearchByProjection(cur, K, T, T, last, std::vector<uint8_t>(), 7.f, false, owner2);
    std::vector<uint8_t> has(N, 0);
    std::vector<float> mp(3 * N, 0.f);
    int nmatches = 0, nmap = 0;
    for (int j = 0; j < N; ++j)
        if (owner2[j] >= 0) { has[j] = 1; memcpy(&mp[3 * j], &last.pos[3 * owner2[j]], 3 * sizeof(float)); }
    PoseOptimization po(K.fx, K.fy, K.cx, K.cy, K.mbf, inv);
    float T2[16];
    memcpy(T2, T, sizeof(T));
    const int ng = po(cur.handle(), has, mp, T2, out2);
    for (int j = 0; j < N; ++j)
        if (has[j] && !out2[j]) { nmatches++; nmap += last.takes[owner2[j]] != 0; }
    if (nm != r.nsearch || owner != owner2 || ng != r.ngood || memcmp(T2, Tout, sizeof(T2)) || out != out2 || nmatches != r.nmatches ||
        nmap != r.nmatches_map) {
        printf("FAIL one call != two calls: nsearch %d / %d ngood %d / %d counts %d %d / %d %d\n", r.nsearch, nm, r.ngood, ng, r.nmatches,
               r.nmatches_map, nmatches, nmap);
        return 1;
    }

    // TrackLocalMap with that result as its base: every point of the list the frame does not hold yet
    std::vector<uint8_t> bh(N, 0), bt(N, 0);
    std::vector<float> bp(3 * N, 0.f);
    ORBmatcher::PointList pts;
    pts.resize(N, true, true, false);
    for (int i = 0; i < N; ++i) {
        pts.valid[i] = 1; pts.takes[i] = last.takes[i];
        memcpy(&pts.pos[3 * i], &last.pos[3 * i], 3 * sizeof(float));
        memcpy(&pts.desc[32 * i], &last.desc[32 * i], 32);
        const float d = std::sqrt(last.pos[3 * i] * last.pos[3 * i] + last.pos[3 * i + 1] * last.pos[3 * i + 1] + last.pos[3 * i + 2] * last.pos[3 * i + 2]);
        pts.normal[3 * i] = last.pos[3 * i] / d; pts.normal[3 * i + 1] = last.pos[3 * i + 1] / d; pts.normal[3 * i + 2] = last.pos[3 * i + 2] / d;
        pts.minDistance[i] = d * K.mvScaleFactors[kps[i].octave] / K.mvScaleFactors[7]; pts.maxDistance[i] = d * K.mvScaleFactors[kps[i].octave];
    }
    for (int j = 0; j < N; ++j)
        if (owner[j] >= 0 && !out[j]) {
            bh[j] = 1; bt[j] = last.takes[owner[j]]; memcpy(&bp[3 * j], &last.pos[3 * owner[j]], 3 * sizeof(float));
            pts.valid[owner[j]] = 0;
        }
    std::vector<int32_t> lown, lown2;
    std::vector<uint8_t> lout, lout2, occ(N, 0);
    float TL[16];
    const orbm_track_result rl = m.TrackLocalMap(cur, K, inv, Tout, pts, bh, bp, bt, 1.f, lown, lout, TL);
    if (m.status() != ORBX_OK || !rl.tracked || rl.ngood < r.ngood / 2) { printf("FAIL TrackLocalMap status %d ngood %d\n", m.status(), rl.ngood); return 1; }
    for (int j = 0; j < N; ++j) occ[j] = bh[j] && bt[j];
    const int nl = m.SearchLocalPoints(cur, K, Tout, pts, occ, 1.f, lown2);
    std::fill(has.begin(), has.end(), 0);
    nmatches = nmap = 0;
    std::vector<uint8_t> tk(N, 0);
    for (int j = 0; j < N; ++j) {
        if (lown2[j] >= 0) { has[j] = 1; tk[j] = pts.takes[lown2[j]]; memcpy(&mp[3 * j], &pts.pos[3 * lown2[j]], 3 * sizeof(float)); }
        else if (bh[j]) { has[j] = 1; tk[j] = bt[j]; memcpy(&mp[3 * j], &bp[3 * j], 3 * sizeof(float)); }
    }
    memcpy(T2, Tout, sizeof(T2));
    const int ngl = po(cur.handle(), has, mp, T2, lout2);
    for (int j = 0; j < N; ++j)
        if (has[j] && !lout2[j]) { nmatches++; nmap += tk[j] != 0; }
    if (nl != rl.nsearch || lown != lown2 || ngl != rl.ngood || memcmp(T2, TL, sizeof(T2)) || lout != lout2 || nmatches != rl.nmatches ||
        nmap != rl.nmatches_map) {
        printf("FAIL local map: one call != two calls: nsearch %d / %d ngood %d / %d counts %d %d / %d %d\n", rl.nsearch, nl, rl.ngood, ngl,
               rl.nmatches, rl.nmatches_map, nmatches, nmap);
        return 1;
    }
    printf("OK motion model: %d matches, %d good, %d / %d kept; local map: %d new, %d good, %d / %d inliers\n", r.nsearch, r.ngood, r.nmatches,
           r.nmatches_map, rl.nsearch, rl.ngood, rl.nmatches, rl.nmatches_map);
    return 0;
}
