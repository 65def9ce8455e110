// LoopClosing_sim3_hip.cc -- the refinement tail of LoopClosing::ComputeSim3 (src/LoopClosing.cc:311-341) on the device: for every
// candidate whose solver returned a similarity in ONE pass of the loop at :288, SearchBySim3 (:323) and OptimizeSim3 (:326) in one
// library call -- one upload, one host wait, nothing back on the host in between.  Reference-side code: compiles in the ORB_SLAM2_E
// tree, beside ORBmatcher_hip.cc (HipPointList::set lives there).
//
// An attempt has no side effects in the reference: vpMapPointMatches and gScm are locals of the attempt (:313, :325).  The pass is
// therefore split: the loop at :288 first runs pSolver->iterate(5, ...) of every candidate still in the race, keeps the discard
// bookkeeping of :304-308 and collects an attempt per non-empty Scm (:313-322, R / t / s from the solver); then
//     const int k = HipRefineSim3Candidates(mpCurrentKF, attempts, 10, mbFixScale);
// and, for k >= 0, :331-337 with attempts[k] (pKF, gScm, vpMapPointMatches).  k is the first attempt in order with nInliers >= 20: the
// attempt at which the reference breaks.  (The candidates behind it have then iterated five times more than in the reference; their
// solvers are deleted without being read again once bMatch is set.)
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Converter.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
#include "hip_frame.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

struct HipSim3Attempt {
    KeyFrame *pKF;                                  // mvpEnoughConsistentCandidates[i]
    std::vector<MapPoint *> vpMapPointMatches;      // in: the solver's inliers (:313-319); out: as OptimizeSim3 leaves them
    cv::Mat R, t;                                   // GetEstimatedRotation / Translation (CV_32F)
    float s;                                        // GetEstimatedScale
    g2o::Sim3 gScm;                                 // out (:325-326)
    int nInliers;                                   // out: OptimizeSim3's return value
};

// Returns the index of the first attempt with nInliers >= 20, or -1.  Every attempt's outputs are filled.
int HipRefineSim3Candidates(KeyFrame *pCurrentKF, std::vector<HipSim3Attempt> &attempts, float th2, bool bFixScale)
{
    const int P = (int)attempts.size();
    if (P == 0) return -1;
    if (P > 64) throw std::runtime_error("HipRefineSim3Candidates: more than 64 attempts in one pass");
    const std::vector<MapPoint *> vpMapPoints1 = pCurrentKF->GetMapPointMatches();
    const int N1 = (int)vpMapPoints1.size();
    HipPointList p1(N1);
    for (int i = 0; i < N1; ++i) { MapPoint *pMP = vpMapPoints1[i]; if (pMP && !pMP->isBad()) p1.set(i, pMP); }     // ORBmatcher.cc:1351-1357, Optimizer.cc:1496-1498
    float T1w[16];
    HipPose(pCurrentKF->GetPose(), T1w);
    const orbm_view view = {pCurrentKF->fx, pCurrentKF->fy, pCurrentKF->cx, pCurrentKF->cy, pCurrentKF->mb, pCurrentKF->mbf,
                            pCurrentKF->mfLogScaleFactor, pCurrentKF->mnScaleLevels, pCurrentKF->mvScaleFactors.data()};
    const orbm_points q1 = p1.view();
    std::vector<std::vector<MapPoint *> > vpMapPoints2(P);
    std::vector<HipPointList> p2;
    std::vector<orbm_points> q2(P);
    std::vector<std::vector<int32_t> > seed(P), found(P), matches(P);
    std::vector<std::vector<float> > T2w(P, std::vector<float>(16));
    std::vector<orbm_refine_sim3_attempt> flat(P);
    p2.reserve(P);
    for (int k = 0; k < P; ++k) {
        HipSim3Attempt &a = attempts[k];
        vpMapPoints2[k] = a.pKF->GetMapPointMatches();
        const int N2 = (int)vpMapPoints2[k].size();
        p2.push_back(HipPointList(N2));
        for (int i = 0; i < N2; ++i) { MapPoint *pMP = vpMapPoints2[k][i]; if (pMP && !pMP->isBad()) p2[k].set(i, pMP); }
        q2[k] = p2[k].view();
        seed[k].assign(N1 > 0 ? N1 : 1, -1); found[k].assign(N1 > 0 ? N1 : 1, -1); matches[k].assign(N1 > 0 ? N1 : 1, -1);
        for (int i = 0; i < N1 && i < (int)a.vpMapPointMatches.size(); ++i) {           // ORBmatcher.cc:1333-1343, Optimizer.cc:1494
            MapPoint *pMP = a.vpMapPointMatches[i];
            if (!pMP) continue;
            const int idx2 = pMP->GetIndexInKeyFrame(a.pKF);
            seed[k][i] = idx2 >= 0 && idx2 < N2 ? idx2 : -2;
        }
        HipPose(a.pKF->GetPose(), T2w[k].data());
        orbm_refine_sim3_attempt &q = flat[k];
        q.kf2 = a.pKF->mpHipFrame.get(); q.points2 = &q2[k]; q.T2w = T2w[k].data();
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) q.R12[3 * r + c] = a.R.at<float>(r, c); q.t12[r] = a.t.at<float>(r); }
        q.s12 = a.s;
        q.seed12 = seed[k].data(); q.found12 = found[k].data(); q.matches12 = matches[k].data();
    }
    std::vector<int32_t> nfound(P, 0);
    std::vector<orbm_sim3_opt_result> res(P);
    const int rc = orbm_refine_sim3_candidates(pCurrentKF->mpHipFrame.get(), &q1, T1w, &view, pCurrentKF->mvInvLevelSigma2.data(), flat.data(), P, 7.5f,
                                               ORBmatcher::TH_HIGH, th2, bFixScale ? 1 : 0, nfound.data(), res.data());
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_refine_sim3_candidates: ") + orbx_last_error());
    int accepted = -1;
    for (int k = 0; k < P; ++k) {
        HipSim3Attempt &a = attempts[k];
        a.vpMapPointMatches.resize(N1, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < N1; ++i) {
            const int m = matches[k][i];
            if (m == -1) a.vpMapPointMatches[i] = static_cast<MapPoint *>(NULL);        // never matched, or erased by the cut (Optimizer.cc:1580, :1614)
            else if (m >= 0 && seed[k][i] == -1) a.vpMapPointMatches[i] = vpMapPoints2[k][m];   // ORBmatcher.cc:1518
        }                                                                               // (a seed that survived keeps its pointer)
        const orbm_sim3_opt_result &r = res[k];
        a.gScm = g2o::Sim3(Converter::toMatrix3d(a.R), Converter::toVector3d(a.t), a.s);            // :325
        if (r.ncorrespondences - r.nbad >= 10)                                                      // Optimizer.cc:1595: else gScm stays as it came in
            a.gScm = g2o::Sim3(Eigen::Quaterniond(r.q[3], r.q[0], r.q[1], r.q[2]), Eigen::Vector3d(r.t[0], r.t[1], r.t[2]), r.s);   // :1622
        a.nInliers = r.nin;
        if (accepted < 0 && a.nInliers >= 20) accepted = k;                                         // :329
    }
    return accepted;
}

} // namespace ORB_SLAM2
