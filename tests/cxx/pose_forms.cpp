// Both overloads of orbslam_hip::PoseOptimization (include/orbslam_hip.hpp) on one scene, driven by tests/test_gpu_pose_edges.py:
// the vector form (host arrays) and the frame-handle form (a frame built by orbm_frame_create from the same keypoints).
//   pose_forms SCENE OUT     runs both and writes, for each form in that order: int32 ngood, float Tcw[16] (the pose the class
//                            left in Tcw), uint8 outlier[n], the orbm_pose_stats bytes.  Exit status 0, or 1 on any error.
// SCENE (raw little-endian): int32 n, nlevels, stereo; float fx fy cx cy mbf, invLevelSigma2[nlevels], Tcw[16], bounds[4] (the
// frame's min_x min_y max_x max_y); float xy[n][2]; int32 octave[n]; float uright[n] (only if stereo); uint8 hasMp[n];
// float mpPos[n][3].
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

namespace {

template <typename T>
bool readv(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

void writeResult(FILE *f, int ngood, const float T[16], const std::vector<uint8_t> &outlier, const orbm_pose_stats &st)
{
    const int32_t g = ngood;
    std::fwrite(&g, sizeof(g), 1, f);
    std::fwrite(T, sizeof(float), 16, f);
    std::fwrite(outlier.data(), 1, outlier.size(), f);
    std::fwrite(&st, sizeof(st), 1, f);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 1;
    std::vector<int32_t> hdr, oct;
    std::vector<float> head, xy, ur, pos;
    std::vector<uint8_t> has;
    if (!readv(in, hdr, 3)) return 1;
    const int n = hdr[0], nlevels = hdr[1], stereo = hdr[2];
    if (!readv(in, head, 5 + nlevels + 16 + 4) || !readv(in, xy, 2 * (size_t)n) || !readv(in, oct, n) ||
        (stereo && !readv(in, ur, n)) || !readv(in, has, n) || !readv(in, pos, 3 * (size_t)n))
        return 1;
    std::fclose(in);
    const float *cam = head.data(), *inv = cam + 5, *Tin = inv + nlevels, *bounds = Tin + 16;

    std::vector<orbx_keypoint> kps(n);
    std::memset(kps.data(), 0, sizeof(orbx_keypoint) * (size_t)n);
    for (int i = 0; i < n; ++i) { kps[i].x = xy[2 * i]; kps[i].y = xy[2 * i + 1]; kps[i].octave = oct[i]; }
    orbslam_hip::PoseOptimization po(cam[0], cam[1], cam[2], cam[3], cam[4], std::vector<float>(inv, inv + nlevels));

    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 1;
    float T[16];
    std::vector<uint8_t> outlier;
    orbm_pose_stats st;

    std::memcpy(T, Tin, sizeof(T));
    std::memset(&st, 0, sizeof(st));
    int ng = po(kps, ur, has, pos, T, outlier, &st);
    if (ng < 0) { std::printf("vector form: status %d\n", po.status()); return 1; }
    writeResult(out, ng, T, outlier, st);

    orbm_frame *frame = nullptr;
    std::vector<uint8_t> desc(32 * (size_t)n, 0);
    if (orbm_frame_create(kps.data(), desc.data(), n, stereo ? ur.data() : nullptr, bounds[0], bounds[1], bounds[2], bounds[3], &frame) !=
        ORBX_OK) {
        std::printf("orbm_frame_create: %s\n", orbx_last_error());
        return 1;
    }
    std::memcpy(T, Tin, sizeof(T));
    std::memset(&st, 0, sizeof(st));
    outlier.clear();
    ng = po(frame, has, pos, T, outlier, &st);
    orbm_frame_destroy(frame);
    if (ng < 0) { std::printf("frame form: status %d\n", po.status()); return 1; }
    writeResult(out, ng, T, outlier, st);
    std::fclose(out);
    std::printf("OK\n");
    return 0;
}
