// Optimizer_sim3_hip.cc -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1430-1625) on the device: the shell does the pointer walk of
// :1483-1520 (through the accessors' own locks, as the reference does), hands the correspondences it keeps to ONE library call that
// runs both optimisation rounds, the cut between them and the final count (:1564-1624), and writes vpMatches1 and g2oS12 back.
// Reference-side code: compiles in the ORB_SLAM2_E tree.  INTEGRATION.md: the body of Optimizer::OptimizeSim3 becomes
// `return HipOptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);`.
//
// The library takes the start as LoopClosing.cc:320-325 forms it, R, t and s in float.  g2oS12 holds that rotation as a quaternion:
// its matrix rounded back to float is the caller's cv::Mat up to the last bit of a float.
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

int HipOptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, float th2, bool bFixScale)
{
    const cv::Mat T1w = pKF1->GetPose().clone(), T2w = pKF2->GetPose().clone();     // 4 x 4 CV_32F, continuous after clone()
    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<float> X1w, X2w, obs1, obs2;
    std::vector<int32_t> octave1, octave2;
    std::vector<size_t> vnIndexEdge;
    for (int i = 0; i < N; i++) {                                                   // :1483-1520
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        const cv::Mat P1 = pMP1->GetWorldPos(), P2 = pMP2->GetWorldPos();
        for (int r = 0; r < 3; r++) { X1w.push_back(P1.at<float>(r)); X2w.push_back(P2.at<float>(r)); }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i], &kpUn2 = pKF2->mvKeysUn[i2];
        obs1.push_back(kpUn1.pt.x); obs1.push_back(kpUn1.pt.y);
        obs2.push_back(kpUn2.pt.x); obs2.push_back(kpUn2.pt.y);
        octave1.push_back(kpUn1.octave); octave2.push_back(kpUn2.octave);
        vnIndexEdge.push_back(i);
    }
    orbm_sim3_opt_problem q;
    q.X1w = X1w.data(); q.X2w = X2w.data(); q.obs1 = obs1.data(); q.obs2 = obs2.data();
    q.octave1 = octave1.data(); q.octave2 = octave2.data();
    q.Tcw1 = T1w.ptr<float>(); q.Tcw2 = T2w.ptr<float>();
    q.fx1 = pKF1->fx; q.fy1 = pKF1->fy; q.cx1 = pKF1->cx; q.cy1 = pKF1->cy;        // = mK (:1458-1465)
    q.fx2 = pKF2->fx; q.fy2 = pKF2->fy; q.cx2 = pKF2->cx; q.cy2 = pKF2->cy;
    const Eigen::Matrix3d R = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) q.R12[3 * r + c] = (float)R(r, c);
        q.t12[r] = (float)g2oS12.translation()[r];
    }
    q.s12 = (float)g2oS12.scale();
    q.th2 = th2;
    q.fix_scale = bFixScale ? 1 : 0;
    q.n = (int32_t)vnIndexEdge.size();
    orbm_sim3_opt_result res;
    std::vector<uint8_t> kept(vnIndexEdge.size() + 1, 0);
    const int rc = orbm_optimize_sim3(&q, 1, pKF1->mvInvLevelSigma2.data(), (int)pKF1->mvInvLevelSigma2.size(), &res, kept.data());
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_optimize_sim3: ") + orbx_last_error());
    for (size_t k = 0; k < vnIndexEdge.size(); k++)                                 // :1580, :1614
        if (!kept[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);
    if (res.ncorrespondences - res.nbad < 10) return 0;                             // :1595: g2oS12 stays as it came in
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(res.q[3], res.q[0], res.q[1], res.q[2]), Eigen::Vector3d(res.t[0], res.t[1], res.t[2]), res.s);   // :1622
    return res.nin;
}

} // namespace ORB_SLAM2
