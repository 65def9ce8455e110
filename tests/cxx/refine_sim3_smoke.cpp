// orbslam_hip::RefineSim3Candidates on a batch that tests/test_gpu_refine_sim3.py wrote to a file: the C++ wrapper's outputs go back to
// a file, byte for byte, for the comparison with the Python call's.  "nodevice": no frame can be made, which must be reported.
//
// File (little endian): int32 P, n1, nlevels, fix_scale; float cam[4], log_sf, th, th2; float sf[nlevels], isg[nlevels];
// KF1: keypoints [n1] (orbx_keypoint), desc [n1][32], valid [n1], pos [n1][3], mind [n1], maxd [n1], T1w[16];
// per attempt: int32 n2; keypoints, desc2 [n2][32]; valid, pos, mind, maxd, mp_desc [n2][32]; T2w[16], R12[9], t12[3], s12; seed [n1].
// Output: per attempt found12 [n1], nfound, matches12 [n1], orbm_sim3_opt_result; then int32 accepted.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

static FILE *g_in;
template <typename T> static std::vector<T> rd(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) { printf("FAIL short read\n"); exit(1); }
    return v;
}
template <typename T> static T rd1() { return rd<T>(1)[0]; }

struct KeyFrame {
    std::vector<orbx_keypoint> kps;
    std::vector<uint8_t> desc;
    ORBmatcher::PointList pts;
    ORBmatcher::ResidentFrame frame;
    void read(int n)
    {
        kps = rd<orbx_keypoint>(n); desc = rd<uint8_t>((size_t)32 * n);
        pts.valid = rd<uint8_t>(n); pts.pos = rd<float>((size_t)3 * n); pts.minDistance = rd<float>(n); pts.maxDistance = rd<float>(n);
        pts.desc = rd<uint8_t>((size_t)32 * n);
        ORBmatcher::FrameView fv;
        fv.mvKeysUn = kps.data(); fv.mDescriptors = desc.data(); fv.N = n; fv.mnMinX = 0.f; fv.mnMinY = 0.f; fv.mnMaxX = 640.f; fv.mnMaxY = 480.f;
        frame = ORBmatcher::ResidentFrame(fv);
    }
};

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "nodevice")) {
        orbx_keypoint k = orbx_keypoint();
        uint8_t d[32] = {0};
        ORBmatcher::FrameView fv;
        fv.mvKeysUn = &k; fv.mDescriptors = d; fv.N = 1; fv.mnMaxX = 640.f; fv.mnMaxY = 480.f;
        ORBmatcher::ResidentFrame f(fv);
        if (f.status() != ORBX_ERR_NO_DEVICE) { printf("FAIL status %d\n", f.status()); return 1; }
        std::vector<RefineSim3Attempt> none;
        ORBmatcher::PointList p; ORBmatcher::Calibration K;
        int accepted = 7;
        if (RefineSim3Candidates(f, p, nullptr, K, std::vector<float>(), none, false, &accepted) != ORBX_OK || accepted != -1) { printf("FAIL empty pass\n"); return 1; }
        printf("OK nodevice\n");
        return 0;
    }
    if (argc != 3 || !(g_in = fopen(argv[1], "rb"))) { printf("usage: refine_sim3_smoke IN OUT | nodevice\n"); return 2; }
    const int P = rd1<int32_t>(), n1 = rd1<int32_t>(), nlevels = rd1<int32_t>(), fix = rd1<int32_t>();
    const std::vector<float> cam = rd<float>(4);
    const float log_sf = rd1<float>(), th = rd1<float>(), th2 = rd1<float>();
    ORBmatcher::Calibration K;
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mfLogScaleFactor = log_sf; K.mvScaleFactors = rd<float>(nlevels);
    const std::vector<float> isg = rd<float>(nlevels);
    KeyFrame kf1;
    kf1.read(n1);
    const std::vector<float> T1w = rd<float>(16);
    std::vector<KeyFrame> kf2((size_t)P);
    std::vector<RefineSim3Attempt> att((size_t)P);
    for (int p = 0; p < P; ++p) {
        kf2[p].read(rd1<int32_t>());
        if (kf2[p].frame.status() != ORBX_OK) { printf("FAIL frame %d: %s\n", p, orbx_last_error()); return 1; }
        att[p].KF2 = &kf2[p].frame; att[p].points2 = &kf2[p].pts;
        memcpy(att[p].T2w, rd<float>(16).data(), sizeof(att[p].T2w)); memcpy(att[p].R12, rd<float>(9).data(), sizeof(att[p].R12));
        memcpy(att[p].t12, rd<float>(3).data(), sizeof(att[p].t12)); att[p].s12 = rd1<float>();
        att[p].seed12 = rd<int32_t>(n1);
    }
    fclose(g_in);
    int accepted = -2;
    const int rc = RefineSim3Candidates(kf1.frame, kf1.pts, T1w.data(), K, isg, att, fix != 0, &accepted, th, th2);
    if (rc != ORBX_OK) { printf("FAIL %d: %s\n", rc, orbx_last_error()); return 1; }
    if (orbm_debug_last_refine_sim3_waits() != 1) { printf("FAIL waits %d\n", orbm_debug_last_refine_sim3_waits()); return 1; }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int p = 0; p < P; ++p) {
        const int32_t nf = att[p].nFound;
        fwrite(att[p].found12.data(), sizeof(int32_t), n1, out); fwrite(&nf, sizeof(nf), 1, out);
        fwrite(att[p].matches12.data(), sizeof(int32_t), n1, out); fwrite(&att[p].result, sizeof(orbm_sim3_opt_result), 1, out);
    }
    const int32_t acc = accepted;
    fwrite(&acc, sizeof(acc), 1, out);
    fclose(out);
    printf("OK %d attempts, accepted %d\n", P, accepted);
    return 0;
}
