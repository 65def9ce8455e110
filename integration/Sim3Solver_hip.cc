// integration/Sim3Solver_hip.cc -- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over orbslam_hip::Sim3Solver: the shell
// walks the pointer graph of the two keyframes on the host (what the constructor keeps of vpMatched12, :43-103), hands the flat
// problem to the library class with DUtils::Random::RandomInt as the source of draws, and turns the results back into cv::Mat.
// Every RANSAC hypothesis of a candidate is then ONE library call (orbm_sim3_hypotheses, at the first iterate()), and every
// iterate() the reference's fold over the stored inlier counts.  LoopClosing.cc is not edited.
//
// Goes to src/Sim3Solver_hip.cc in place of src/Sim3Solver.cc in the reference's CMakeLists.txt.  Like the other shells it cannot
// be compiled where OpenCV / DBoW2 are absent, and reference.patch does not carry it (its hunks are pinned).  The class keeps its
// header: the library object of a solver lives in a table keyed by the solver's address (LoopClosing never deletes its solvers,
// src/LoopClosing.cc:262-275, so neither does the table).
//
// One difference to the reference: the draws of one solver are made together, at its first iterate(); in
// LoopClosing::ComputeSim3 they interleave with the other candidates' draws in five-iteration rounds.  Results equal the reference
// run whose RNG hands each solver these triples (the reference seeds nothing here).  To evaluate all candidates of a loop
// detection in one launch, call Sim3SolverHipEvaluateBatch(vpSim3Solvers) in front of the round-robin of :288.
#include "Sim3Solver.h"

#include <iostream>
#include <map>
#include <memory>
#include <mutex>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbslam_hip.hpp"

namespace ORB_SLAM2
{

namespace
{
std::mutex gTableMutex;
std::map<const Sim3Solver *, std::unique_ptr<orbslam_hip::Sim3Solver> > gTable;

orbslam_hip::Sim3Solver *HipOf(const Sim3Solver *p)
{
    std::unique_lock<std::mutex> lock(gTableMutex);
    std::map<const Sim3Solver *, std::unique_ptr<orbslam_hip::Sim3Solver> >::iterator it = gTable.find(p);
    return it == gTable.end() ? NULL : it->second.get();
}

int DrawInt(int lo, int hi) { return DUtils::Random::RandomInt(lo, hi); }

void CopyPose(const cv::Mat &T, float *out)
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = T.at<float>(r, c);
}

cv::Mat ToMat(const float *v, int rows, int cols)
{
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<float>(r, c) = v[cols * r + c];
    return m;
}
}

// The first evaluation of every solver of a loop detection in one library call (up to 64 candidates per launch)
void Sim3SolverHipEvaluateBatch(const std::vector<Sim3Solver *> &vpSolvers)
{
    std::vector<orbslam_hip::Sim3Solver *> v;
    for (size_t i = 0; i < vpSolvers.size(); ++i)
        if (vpSolvers[i]) v.push_back(HipOf(vpSolvers[i]));
    if (orbslam_hip::Sim3Solver::EvaluateBatch(v) != ORBX_OK) std::cerr << "Sim3Solver: " << orbx_last_error() << std::endl;
}

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const vector<MapPoint *> &vpMatched12, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
{
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    mvpMatches12 = vpMatched12;
    mN1 = (int)vpMatched12.size();

    orbslam_hip::Sim3Solver::Problem flat;
    flat.N1 = mN1;
    flat.bFixScale = bFixScale;
    flat.levelSigma2 = pKF1->mvLevelSigma2;                    // one pyramid: the keyframes of a map share the extractor
    CopyPose(pKF1->GetPose(), flat.Tcw1);
    CopyPose(pKF2->GetPose(), flat.Tcw2);
    flat.fx1 = pKF1->fx; flat.fy1 = pKF1->fy; flat.cx1 = pKF1->cx; flat.cy1 = pKF1->cy;
    flat.fx2 = pKF2->fx; flat.fy2 = pKF2->fy; flat.cx2 = pKF2->cx; flat.cy2 = pKF2->cy;

    // the pairs the reference keeps (:62-103): both points exist, neither is bad, both are observed in their keyframe
    const vector<MapPoint *> vpOwn = pKF1->GetMapPointMatches();
    for (int i1 = 0; i1 < mN1; ++i1) {
        MapPoint *pMP2 = vpMatched12[i1];
        MapPoint *pMP1 = pMP2 ? vpOwn[i1] : NULL;
        if (!pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
        const int idx1 = pMP1->GetIndexInKeyFrame(pKF1), idx2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (idx1 < 0 || idx2 < 0) continue;
        const cv::Mat x1 = pMP1->GetWorldPos(), x2 = pMP2->GetWorldPos();
        for (int r = 0; r < 3; ++r) { flat.X1w.push_back(x1.at<float>(r)); flat.X2w.push_back(x2.at<float>(r)); }
        flat.octave1.push_back(pKF1->mvKeysUn[idx1].octave);
        flat.octave2.push_back(pKF2->mvKeysUn[idx2].octave);
        flat.indices1.push_back(i1);
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
    }
    N = (int)mvpMapPoints1.size();
    mK1 = pKF1->mK;
    mK2 = pKF2->mK;
    {
        std::unique_lock<std::mutex> lock(gTableMutex);
        gTable[this].reset(new orbslam_hip::Sim3Solver(std::move(flat), &DrawInt));
    }
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    orbslam_hip::Sim3Solver *hip = HipOf(this);
    hip->SetRansacParameters(probability, minInliers, maxIterations);
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = hip->GetRansacMaxIts();
    mnIterations = 0;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    orbslam_hip::Sim3Solver *hip = HipOf(this);
    float T12[16];
    const bool found = hip->iterate(nIterations, bNoMore, vbInliers, nInliers, T12);
    if (hip->status() != ORBX_OK) std::cerr << "Sim3Solver: " << orbx_last_error() << std::endl;
    if (!found) return cv::Mat();
    mBestT12 = ToMat(T12, 4, 4);
    return mBestT12;
}

cv::Mat Sim3Solver::find(vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    float R[9];
    return HipOf(this)->GetEstimatedRotation(R) ? ToMat(R, 3, 3) : cv::Mat();
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    float t[3];
    return HipOf(this)->GetEstimatedTranslation(t) ? ToMat(t, 3, 1) : cv::Mat();
}

float Sim3Solver::GetEstimatedScale()
{
    return HipOf(this)->GetEstimatedScale();
}

} // namespace ORB_SLAM2
