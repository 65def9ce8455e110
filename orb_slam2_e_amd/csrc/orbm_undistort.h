// orbm_undistort.h -- Frame::UndistortKeyPoints / ComputeImageBounds (src/Frame.cc:419-479): one keypoint through
// cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) as OpenCV 3.4 evaluates it for CV_32FC2 points (cvUndistortPointsInternal:
// double arithmetic, five fixed-point iterations of the inverse distortion, no tilt, no rational / thin-prism terms for a 4- or
// 5-entry mDistCoef).  ONE definition for the host (orbm_image_bounds) and the device (k_frame_build, k_undistort_points): the
// library is built with -ffp-contract=off, and IEEE double + - * / give the same bits on both.  Parity UNPINNED.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/orbslam_hip.h"

namespace orbm_detail {

// mvKeysUn[i].pt of the keypoint at (px, py).  k1 == 0: the keypoint itself (Frame.cc:421-425 tests mDistCoef.at<float>(0) only).
// Near the border of a wide-angle image the iteration diverges (huge or non-finite results): the reference stores those too.
__host__ __device__ inline void undistort_point(const orbm_distortion &c, float px, float py, float *u, float *v)
{
    if (c.k1 == 0.0f) { *u = px; *v = py; return; }
    const double fx = (double)c.fx, fy = (double)c.fy, cx = (double)c.cx, cy = (double)c.cy;
    const double k1 = (double)c.k1, k2 = (double)c.k2, p1 = (double)c.p1, p2 = (double)c.p2, k3 = (double)c.k3;
    const double ifx = 1.0 / fx, ify = 1.0 / fy;
    const double x0 = ((double)px - cx) * ifx, y0 = ((double)py - cy) * ify;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    *u = (float)(fx * x + cx);
    *v = (float)(fy * y + cy);
}

// every field finite, fx and fy not 0 (what the entry points refuse otherwise)
inline bool distortion_ok(const orbm_distortion &c)
{
    const float f[9] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3};
    for (float v : f)
        if (!isfinite(v)) return false;
    return c.fx != 0.0f && c.fy != 0.0f;
}

} // namespace orbm_detail
