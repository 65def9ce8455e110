// Optimizer_pose_nr_hip.cc -- the bundle of Optimizer::PoseOptimizationNR (src/Optimizer.cc:478-834) on the device.  The walk over
// MapPoint* / KeyFrame* (:515-709) stays here, on the host, and fills a flat graph instead of a g2o::SparseOptimizer; fea2.Compute(1)
// (:723, with integration/FEA2_hip.cc: assembly, Dirichlet penalty and fem_trial_setup on fea2.mFem) is the reference's call; the
// non-linear optimisation, the inlier / outlier passes and the write-back (:733-809) are ONE call of orbm_pose_optimization_nr.
// Reference-side code: compiles in the ORB_SLAM2_E tree.  INTEGRATION.md: Optimizer::PoseOptimizationNR keeps its declarations
// (:480-481, fea2) and its tail (:830-833) and replaces :483-809 with
//     int nBadOrError = HipPoseOptimizationNR(pFrame, pMap, pFrameDrawer, fea2);
// Three things of :483-809 are NOT reproduced, each for its stated reason:
//   :558-594  the other map points inside the frustum, collected into vpMPsInFrame (never read) and fea2.vpMPs_ut (read only by the
//             dead Compute(2) block, :812-828): left out with that block;
//   :673-699  the edge to the mnId == 0 keyframe, which has no vertex (:533): optimizer.vertex(0) is the FRAME's pose there;
//   :764      `if (pMP->isBad()) continue;` inside the inlier / outlier pass: the pass runs inside the launch on the graph as it was
//             flattened, so a map point another thread marks bad WHILE the call runs is classified like the others (the reference
//             would leave its flags as they were).  Points that are bad before the call are not in mvpMapPoints' matches to begin with.
// A problem beyond the kernel's limits (ORBX_ERR_UNSUPPORTED: more than 1,365 top-layer nodes, 65,536 edges or 1,024 keyframes)
// returns -2: the caller then runs the reference's own g2o loop, whose hook FEA2_hip.cc serves one trial at a time.
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "FEA2.h"
#include "Frame.h"
#include "FrameDrawer.h"
#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "fem_hip.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

static void push_pose(std::vector<float> &dst, const cv::Mat &T)       // 4 x 4 CV_32F, row-major
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) dst.push_back(T.at<float>(r, c));
}

// Returns nInitialCorrespondences - nBad (:833), 0 where the reference returns 0 (:711-714, :728-729), -2 beyond the kernel's limits.
int HipPoseOptimizationNR(Frame *pFrame, Map *pMap, FrameDrawer *pFrameDrawer, FEA2 &fea2)
{
    // ---- :515-556: the matched map points and the fixed keyframes that observe them (the mnId == 0 keyframe gets no vertex, :533)
    std::vector<MapPoint *> vpMapPoints;
    std::vector<cv::KeyPoint> vKeysUn;
    std::vector<KeyFrame *> vpFixedKFs;
    std::map<KeyFrame *, int32_t> kfIndex;
    std::vector<float> kfTcw;
    for (size_t i = 0; i < pFrame->mvpMapPoints.size(); i++) {
        MapPoint *pMP = pFrame->mvpMapPoints[i];
        if (!pMP) continue;
        pMP->bSetForReloc = true;
        vpMapPoints.push_back(pMP);
        vKeysUn.push_back(pFrame->mvKeysUn[i]);
        fea2.vpKPs_t.push_back(&pFrame->mvKeys[i]);
        fea2.vpMPs_t.push_back(pMP);
        fea2.vpMPs_ut.push_back(pMP);
        fea2.idxMpF.push_back(i);
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->mnId == 0 || pKFi->isBad() || pKFi->mnBAFixedForReloc == pFrame->mnId) continue;
            pKFi->mnBAFixedForReloc = pFrame->mnId;
            kfIndex[pKFi] = (int32_t)vpFixedKFs.size();
            vpFixedKFs.push_back(pKFi);
            push_pose(kfTcw, pKFi->GetPose());
        }
    }
    // (:558-594 is left out: see the head of this file)
    for (size_t i = 0; i < vpFixedKFs.size(); i++) vpFixedKFs[i]->mnBAFixedForReloc = 0;      // :596-598

    // ---- :619-709: one point vertex per matched map point, its frame edge, then its keyframe edges -- the order the kernel wants
    // (edges grouped by point, the frame edge first)
    const int n = (int)vpMapPoints.size();
    std::vector<float> points(3 * (size_t)n), eObs, eInv, eK;
    std::vector<int32_t> ePoint, eCam;
    for (int i = 0; i < n; i++) {
        MapPoint *pMP = vpMapPoints[i];
        const cv::Mat Xw = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) points[3 * i + k] = Xw.at<float>(k);
        pFrame->mvbOutlier[i] = false;                                   // :632 (indexed as the reference indexes it)
        const cv::KeyPoint &kpUn = vKeysUn[i];
        const float invSigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
        ePoint.push_back(i); eCam.push_back(-1);
        eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y);
        eInv.push_back(invSigma2);
        eK.push_back(pFrame->fx); eK.push_back(pFrame->fy); eK.push_back(pFrame->cx); eK.push_back(pFrame->cy);
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
            KeyFrame *pKFi = mit->first;
            if (!pKFi || pKFi->isBad()) continue;                        // :673
            // The reference builds an edge to the mnId == 0 keyframe too (:673-699) although that keyframe never got a vertex (:533):
            // optimizer.vertex(0) is the FRAME's pose there.  That edge is left out here, as is one to a keyframe without a vertex.
            const std::map<KeyFrame *, int32_t>::const_iterator at = kfIndex.find(pKFi);
            if (at == kfIndex.end()) continue;
            const cv::KeyPoint kpUn2 = pKFi->GetKeyPointUn(mit->second);
            ePoint.push_back(i); eCam.push_back(at->second);
            eObs.push_back(kpUn2.pt.x); eObs.push_back(kpUn2.pt.y);
            eInv.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);       // :684-685: the FRAME keypoint's octave
            eK.push_back(pKFi->fx); eK.push_back(pKFi->fy); eK.push_back(pKFi->cx); eK.push_back(pKFi->cy);
        }
    }
    if (n < 3) return 0;                                                 // :711-714

    // ---- :723: the mesh, K, the Dirichlet penalty and the hook's state on the device (FEA2_hip.cc); fea2.vVertices is not needed:
    // the kernel's point i IS vpMapPoints[i]
    if (!fea2.Compute(1)) return 0;                                          // :728-729
    pMap->vpMPs2Draw = fea2.vpMPs2Draw;                                      // :724-726
    pFrameDrawer->vpKPs2Draw = fea2.vpKPs2Draw;
    pFrameDrawer->vpMPs2Draw = fea2.vpMPs2Draw;

    // ---- :733-809 in one call
    cv::Mat Tin = pFrame->mTcw.clone();
    orbm_pose_nr_graph g;
    g.npoints = n; g.nkf = (int32_t)vpFixedKFs.size(); g.nedges = (int32_t)ePoint.size(); g.reserved = 0;
    g.Tcw = Tin.ptr<float>(); g.kf_Tcw = kfTcw.data(); g.points = points.data(); g.e_point = ePoint.data(); g.e_cam = eCam.data();
    g.e_obs = eObs.data(); g.e_inv_sigma2 = eInv.data(); g.e_cam_k = eK.data();
    std::vector<float> pointsOut(3 * (size_t)n);
    std::vector<uint8_t> outlier(n, 0);
    orbm_pose_nr_result res;
    res.points_out = pointsOut.data(); res.outlier = outlier.data(); res.ngood = 0; res.reserved = 0;
    const int rc = orbm_pose_optimization_nr(fea2.mFem, &g, &res, nullptr);
    if (rc == ORBX_ERR_UNSUPPORTED) return -2;
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_pose_optimization_nr: ") + orbx_last_error());

    for (int i = 0; i < n; i++) pFrame->mvbOutlier[i] = outlier[i] != 0;     // :769, :779 (bRelocCheck is back at true: :791-795)
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = res.Tcw[4 * r + c];
    pFrame->SetPose(pose);                                                   // :798-801
    for (int i = 0; i < n; i++) {                                            // :804-809
        cv::Mat Xw(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) Xw.at<float>(k) = pointsOut[3 * i + k];
        vpMapPoints[i]->SetWorldPos(Xw);
    }
    return res.ngood;                                                        // :833
}

} // namespace ORB_SLAM2
