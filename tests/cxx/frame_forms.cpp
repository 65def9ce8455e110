// The ResidentFrame forms that take a camera, from C++ (include/orbslam_hip.hpp), built and run by tests/test_gpu_frame_undistort.py /
// tests/test_cpu_undistort.py.  argv[1] = a scene written by the test (ints B, height, width, nfeatures; nine camera floats; four
// bounds; then B images), argv[2] = where the results go, per frame: int n, int nsorted, perm[nsorted], mvKeysUn xy[n][2] -- first
// the constructor form (frame 0), then every frame of FromBatch(0, B).
// argv[1] = "nodevice": ImageBounds works, the frame-making forms fail loudly.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

static bool put(FILE *o, const ORBmatcher::ResidentFrame &F)
{
    int n = 0, ns = 0;
    if (F.status() != ORBX_OK || orbm_frame_size(F.handle(), &n, &ns) != ORBX_OK || n != F.N) return false;
    std::vector<int32_t> perm((size_t)ns + 1);
    if (orbm_frame_layout(F.handle(), perm.data(), nullptr) != ORBX_OK) return false;
    const std::vector<float> xy = F.KeysUn();
    if (xy.size() != (size_t)2 * n) return false;
    const int32_t hdr[2] = {n, ns};
    fwrite(hdr, sizeof(int32_t), 2, o);
    fwrite(perm.data(), sizeof(int32_t), ns, o);
    fwrite(xy.data(), sizeof(float), xy.size(), o);
    return true;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "nodevice")) {
        ORBmatcher::Distortion cam;
        cam.fx = 500.f; cam.fy = 500.f; cam.cx = 320.f; cam.cy = 240.f; cam.k2 = 0.5f;      // k1 == 0: no undistortion
        float b[4] = {-1.f, -1.f, -1.f, -1.f};
        if (ORBmatcher::ImageBounds(cam, 640, 480, b[0], b[1], b[2], b[3]) != ORBX_OK || b[0] != 0.f || b[1] != 0.f || b[2] != 640.f || b[3] != 480.f) {
            printf("FAIL bounds %g %g %g %g\n", b[0], b[1], b[2], b[3]);
            return 1;
        }
        ORBextractor ex(500, 1.2f, 8, 20, 7);
        int status = ORBX_OK;
        std::vector<ORBmatcher::ResidentFrame> fs = ORBmatcher::ResidentFrame::FromBatch(ex, 0, 1, &cam, false, 0.f, 0.f, 640.f, 480.f, &status);
        ORBmatcher::ResidentFrame one(ex, cam, nullptr, false, 0.f, 0.f, 640.f, 480.f);
        if (!fs.empty() || status == ORBX_OK || one.status() == ORBX_OK || one.handle() || !one.KeysUn().empty()) {
            printf("FAIL status %d %d\n", status, one.status());
            return 1;
        }
        printf("OK nodevice\n");
        return 0;
    }
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4]; float c[9], bnd[4];
    if (fread(hdr, 4, 4, f) != 4 || fread(c, 4, 9, f) != 9 || fread(bnd, 4, 4, f) != 4) return 2;
    const int B = hdr[0], h = hdr[1], w = hdr[2];
    std::vector<uint8_t> images((size_t)B * h * w);
    if (fread(images.data(), 1, images.size(), f) != images.size()) return 2;
    fclose(f);
    ORBmatcher::Distortion cam;
    cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3]; cam.k1 = c[4]; cam.k2 = c[5]; cam.p1 = c[6]; cam.p2 = c[7]; cam.k3 = c[8];
    ORBextractor ex(hdr[3], 1.2f, 8, 20, 7);
    if (ex.status() != ORBX_OK || orbx_reserve(ex.handle(), w, h, B) != ORBX_OK ||
        orbx_extract_batch(ex.handle(), images.data(), 0, w, h, w, (size_t)w * h, B, nullptr) != ORBX_OK) {
        printf("FAIL extraction: %s\n", orbx_last_error());
        return 1;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    ORBmatcher::ResidentFrame one(ex, cam, nullptr, false, bnd[0], bnd[1], bnd[2], bnd[3]);
    if (!put(o, one)) { printf("FAIL constructor form %d: %s\n", one.status(), orbx_last_error()); return 1; }
    int status = ORBX_OK;
    std::vector<ORBmatcher::ResidentFrame> fs = ORBmatcher::ResidentFrame::FromBatch(ex, 0, B, &cam, false, bnd[0], bnd[1], bnd[2], bnd[3], &status);
    if (status != ORBX_OK || (int)fs.size() != B) { printf("FAIL batch form %d: %s\n", status, orbx_last_error()); return 1; }
    for (const ORBmatcher::ResidentFrame &F : fs)
        if (!put(o, F)) { printf("FAIL batch frame: %s\n", orbx_last_error()); return 1; }
    fclose(o);
    printf("OK %d frames\n", B);
    return 0;
}
