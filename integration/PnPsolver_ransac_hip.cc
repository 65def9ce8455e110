// integration/PnPsolver_ransac_hip.cc -- the EPnP RANSAC of PnPsolver (src/PnPsolver.cc) over orbslam_hip::PnPsolver: the original
// iterate (:170-263), and the first stage of the fork's iterate(Frame &, .., Map *) (:298-401), as folds over ONE library call each
// (orbm_pnp_hypotheses: compute_pose and CheckInliers of every drawn set, and the Refine behind every new best).  The second stage
// of the fork's function stays with integration/PnPsolver_hip.cc (PnPsolverHipProjectBestPoses), to which this file hands the
// recorded poses in the arrays the reference's histogram code (:419-476) reads.
//
// Goes to src/PnPsolver_ransac_hip.cc beside src/PnPsolver.cc and src/PnPsolver_hip.cc in the reference's CMakeLists.txt.  The
// class keeps its header and PnPsolver.cc keeps its members; four places of it call in here (relocalisation):
//   the constructor's end (:111)        PnPsolverHipRegister(this, F, mvKeyPointIndices, mvP3Dw, mvP2D, vpMapPointMatches.size());
//   SetRansacParameters' end (:158)     PnPsolverHipSetRansacParameters(this, probability, minInliers, maxIterations, minSet, epsilon, th2);
//                                       (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon and mvMaxError are computed as before)
//   iterate (:170-263), the whole body  return PnPsolverHipIterate(this, nIterations, bNoMore, vbInliers, nInliers);
//   iterate(Frame &, ..) (:296-401)     the while loop becomes
//                                         cv::Mat Tcw;
//                                         if (PnPsolverHipIterateFrameStage1(this, rF, snapshot, vpMapPointMatches, nIterations, vbInliers,
//                                                                            nInliers, RPoses, tPoses, inlierPoses, Tcw)) return Tcw;
// reference.patch does not carry these lines (its hunks are pinned).  Like the other shells this file cannot be compiled where
// OpenCV / DBoW2 are absent.  The library object of a solver lives in a table keyed by the solver's address and is dropped by
// PnPsolverHipForget(this) from the destructor.
//
// Differences to the reference, all stated in DESIGN 22: the draws of one solver are made together, when its hypotheses are
// evaluated (in Tracking::Relocalization they interleave with the other candidates' draws in five-iteration rounds); the SVD's
// hypot; Refines behind the one that succeeds are SPECULATIVE -- the reference would not have run them; their results are computed
// in the same call and never read.  They cost device time only.  To evaluate all candidates of a relocalisation in one launch, call
// PnPsolverHipEvaluate(vpPnPsolvers) in front of the round-robin of src/Tracking.cc:1826.
#include "PnPsolver.h"

#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "hip_frame.h"
#include "orbslam_hip.hpp"

using namespace std;

namespace ORB_SLAM2
{

// integration/PnPsolver_hip.cc
struct HipMapSnapshot {
    vector<MapPoint *> vpPoints;
    std::shared_ptr<orbm_map> pMap;
};

namespace
{
std::mutex gTableMutex;
std::map<const PnPsolver *, std::unique_ptr<orbslam_hip::PnPsolver> > gTable;

orbslam_hip::PnPsolver *HipOf(const PnPsolver *p)
{
    std::unique_lock<std::mutex> lock(gTableMutex);
    std::map<const PnPsolver *, std::unique_ptr<orbslam_hip::PnPsolver> >::iterator it = gTable.find(p);
    return it == gTable.end() ? NULL : it->second.get();
}

int DrawInt(int lo, int hi) { return DUtils::Random::RandomInt(lo, hi); }

cv::Mat ToMat(const float *v)
{
    cv::Mat m(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) m.at<float>(r, c) = v[4 * r + c];
    return m;
}

// What the first stage's projection search (:360-364) needs, and what it leaves for :374-384
struct ProjectionSearch {
    Frame *pF;
    const HipMapSnapshot *pSnap;
    vector<int32_t> matched;
    int nMatched;
};

// SearchByProjection(rF, pMap, mRi, mti, .., 15.0) under the refined pose: nMatched >= 12 (:367)
bool AcceptByProjection(const double R[9], const double t[3], void *user)
{
    ProjectionSearch &s = *static_cast<ProjectionSearch *>(user);
    Frame &rF = *s.pF;
    const int nFeatures = (int)rF.mvKeysUn.size();
    s.matched.assign((size_t)nFeatures + 1, -1);
    s.nMatched = 0;
    vector<uint8_t> has(nFeatures + 1, 0);
    for (int j = 0; j < nFeatures; ++j) has[j] = rF.mvpMapPoints[j] != NULL;
    const vector<int> b = rF.GetImageBounds();
    const orbm_camera cam = {Frame::fx, Frame::fy, Frame::cx, Frame::cy, b[0], b[1], b[2], b[3], Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY};
    int32_t nm = 0;
    if (!s.pSnap->pMap || orbm_frame_search_by_projection_map_poses(rF.mpHipFrame.get(), has.data(), s.pSnap->pMap.get(), R, t, 1, &cam,
                                                                    rF.mvScaleFactors.data(), rF.mnScaleLevels, 15.0f, 0.75f, ORBmatcher::TH_RELOC,
                                                                    s.matched.data(), &nm, NULL) != ORBX_OK)
        return false;
    s.nMatched = nm;
    return nm >= 12;
}
}

void PnPsolverHipRegister(const PnPsolver *self, const Frame &F, const vector<size_t> &vKeyPointIndices, const vector<cv::Point3f> &vP3Dw,
                          const vector<cv::Point2f> &vP2D, size_t nMatches)
{
    orbslam_hip::PnPsolver::Problem flat;
    flat.nMatches = (int)nMatches;
    flat.levelSigma2 = F.mvLevelSigma2;
    flat.fu = F.fx; flat.fv = F.fy; flat.uc = F.cx; flat.vc = F.cy;
    for (size_t k = 0; k < vKeyPointIndices.size(); ++k) {
        flat.Xw.push_back(vP3Dw[k].x); flat.Xw.push_back(vP3Dw[k].y); flat.Xw.push_back(vP3Dw[k].z);
        flat.uv.push_back(vP2D[k].x); flat.uv.push_back(vP2D[k].y);
        flat.octave.push_back(F.mvKeysUn[vKeyPointIndices[k]].octave);
        flat.indices.push_back((int32_t)vKeyPointIndices[k]);
    }
    std::unique_lock<std::mutex> lock(gTableMutex);
    gTable[self].reset(new orbslam_hip::PnPsolver(std::move(flat), &DrawInt));
}

void PnPsolverHipForget(const PnPsolver *self)
{
    std::unique_lock<std::mutex> lock(gTableMutex);
    gTable.erase(self);
}

void PnPsolverHipSetRansacParameters(const PnPsolver *self, double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    HipOf(self)->SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2);
}

// The evaluation that the next iterate(nIterations) of every solver needs, in one library call (up to 64 candidates per launch)
void PnPsolverHipEvaluate(const vector<PnPsolver *> &vpSolvers, int nIterations)
{
    vector<orbslam_hip::PnPsolver *> v;
    for (size_t i = 0; i < vpSolvers.size(); ++i)
        if (vpSolvers[i]) v.push_back(HipOf(vpSolvers[i]));
    if (orbslam_hip::PnPsolver::evaluate(v, nIterations) != ORBX_OK) std::cerr << "PnPsolver: " << orbx_last_error() << std::endl;
}

// iterate (:170-263)
cv::Mat PnPsolverHipIterate(const PnPsolver *self, int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    orbslam_hip::PnPsolver *hip = HipOf(self);
    float Tcw[16];
    const bool found = hip->iterate(nIterations, bNoMore, vbInliers, nInliers, Tcw);
    if (hip->status() != ORBX_OK) std::cerr << "PnPsolver: " << orbx_last_error() << std::endl;
    if (!found) {
        vbInliers.clear();              // the reference returns the cleared vector with an empty matrix
        return cv::Mat();
    }
    return ToMat(Tcw);
}

// The while loop of iterate(Frame &, ..) (:298-401).  true: the function returns Tcw (:395) with vbInliers, nInliers and
// vpMapPointMatches set as :370-384 set them.  false: RPoses / tPoses [iteration] and inlierPoses hold what the loop recorded
// (:326-335), for the histogram code and PnPsolverHipProjectBestPoses behind it.
bool PnPsolverHipIterateFrameStage1(const PnPsolver *self, Frame &rF, const HipMapSnapshot &snap, vector<MapPoint *> &vpMapPointMatches,
                                    int nIterations, vector<bool> &vbInliers, int &nInliers, double (*RPoses)[3][3], double (*tPoses)[3],
                                    vector<int> &inlierPoses, cv::Mat &Tcw)
{
    orbslam_hip::PnPsolver *hip = HipOf(self);
    ProjectionSearch search;
    search.pF = &rF; search.pSnap = &snap; search.nMatched = 0;
    std::vector<orbslam_hip::PnPsolver::RecordedPose> poses;
    float T[16];
    const bool found = hip->iterateFrameStage1(nIterations, &AcceptByProjection, &search, vbInliers, nInliers, T, poses);
    if (hip->status() != ORBX_OK) std::cerr << "PnPsolver: " << orbx_last_error() << std::endl;
    for (size_t k = 0; k < poses.size(); ++k) {
        const orbslam_hip::PnPsolver::RecordedPose &p = poses[k];
        for (int i = 0; i < 3; ++i) {
            tPoses[p.iteration][i] = p.t[i];
            for (int j = 0; j < 3; ++j) RPoses[p.iteration][i][j] = p.R[3 * i + j];
        }
        inlierPoses.push_back(p.nInliers);
    }
    if (!found) {
        vbInliers.clear();
        return false;
    }
    const int nFeatures = (int)rF.mvKeysUn.size();
    for (int j = 0; j < nFeatures; ++j)
        if (search.matched[j] >= 0) vpMapPointMatches[j] = snap.vpPoints[search.matched[j]];     // :377-384
    Tcw = ToMat(T);
    return true;
}

} // namespace ORB_SLAM2
