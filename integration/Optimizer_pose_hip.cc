// Optimizer_pose_hip.cc -- Optimizer::PoseOptimization (src/Optimizer.cc:264-476) on the device: the frame is flattened
// (mvKeysUn, mvuRight, mvpMapPoints -> has_mp / world positions, mvInvLevelSigma2) and one library call runs the 4 rounds of the
// g2o graph the reference builds.  Reference-side code: compiles in the ORB_SLAM2_E tree.  INTEGRATION.md 3h: the body of
// Optimizer::PoseOptimization becomes `return HipPoseOptimization(pFrame);`.
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "MapPoint.h"
#include "hip_frame.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

int HipPoseOptimization(Frame *pFrame)
{
    const int N = pFrame->N;
    std::vector<uint8_t> has(N, 0), outlier(N, 0);
    std::vector<float> pos(3 * (size_t)N, 0.f);
    int nmp = 0;
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);            // Optimizer.cc:298
        for (int i = 0; i < N; i++) {
            MapPoint *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            has[i] = 1;
            nmp++;
            const cv::Mat Xw = pMP->GetWorldPos();
            pos[3 * i] = Xw.at<float>(0); pos[3 * i + 1] = Xw.at<float>(1); pos[3 * i + 2] = Xw.at<float>(2);
        }
    }
    orbm_pose_camera cam;
    cam.fx = pFrame->fx; cam.fy = pFrame->fy; cam.cx = pFrame->cx; cam.cy = pFrame->cy; cam.bf = pFrame->mbf;
    cam.nlevels = (int32_t)pFrame->mvInvLevelSigma2.size();
    cam.inv_level_sigma2 = pFrame->mvInvLevelSigma2.data();
    cv::Mat Tin = pFrame->mTcw.clone();                                 // 4 x 4 CV_32F, continuous after clone()
    cv::Mat Tout(4, 4, CV_32F);
    int ngood = 0, rc;
    if (pFrame->mpHipFrame) {
        rc = orbm_frame_pose_optimization(pFrame->mpHipFrame.get(), has.data(), pos.data(), &cam, Tin.ptr<float>(), Tout.ptr<float>(),
                                          outlier.data(), &ngood, nullptr);
    } else {
        std::vector<orbx_keypoint> kps(N);
        for (int i = 0; i < N; i++) {
            const cv::KeyPoint &k = pFrame->mvKeysUn[i];
            kps[i] = orbx_keypoint{k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave, k.class_id};
        }
        rc = orbm_pose_optimization(kps.data(), pFrame->mvuRight.data(), N, has.data(), pos.data(), &cam, Tin.ptr<float>(), Tout.ptr<float>(),
                                    outlier.data(), &ngood, nullptr);
    }
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_pose_optimization: ") + orbx_last_error());
    for (int i = 0; i < N; i++)
        if (has[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;           // Optimizer.cc:312, :405-416
    if (nmp < 3) return 0;                                              // :385-386: the pose stays as it was
    pFrame->SetPose(Tout);                                              // :470-472
    return ngood;
}

} // namespace ORB_SLAM2
