// integration/PnPsolver_hip.cc -- the second stage of the fork's PnPsolver::iterate(Frame&, .., Map*) (src/PnPsolver.cc:488-577) over
// ONE library call.  That stage walks the recorded "best poses" twice (itHist = 0, 1; at most five poses, so at most ten visits,
// several of them under the same pose) and runs the whole-map SearchByProjection at every visit: the same frame, the same map, only
// Rcw / tcw change, and no search reads what another wrote (F.mvpMapPoints is only read; mRelocProj* is read nowhere outside the
// search, so this shell does not fill it and asks for no projections).  Here the distinct poses of the walk are searched together
// (orbm_frame_search_by_projection_map_poses: one upload of a few hundred bytes, one launch, one host wait) and the reference's
// fold is then replayed over the rows in the reference's visiting order: the first visit with more than 30 matches returns, else
// the best of the saved ones.
//
// Searches behind an early return are SPECULATIVE: the reference would not have run them; their rows are computed and discarded.
// They cost device time only (the launch is one either way) and change nothing the caller can see.
//
// The map travels as a snapshot made ONCE per Tracking::Relocalization() (HipMapSnapshotOf) and shared by the iterate() of every
// candidate keyframe; the reference calls pMap->GetAllMapPoints() inside every search.  A map point created or erased by another
// thread during one Relocalization() is therefore seen by all of its searches or by none.
//
// Goes to src/PnPsolver_hip.cc beside src/PnPsolver.cc in the reference's CMakeLists.txt (PnPsolver.cc stays: EPnP, the RANSAC loop
// and its first-stage searches are not replaced).  The hook is described in INTEGRATION.md; reference.patch does not carry it (its
// hunks are pinned).  Like the other shells it cannot be compiled where OpenCV is absent.
#include "PnPsolver.h"

#include <string.h>

#include <memory>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "hip_frame.h"
#include "orbslam_hip.h"

using namespace std;

namespace ORB_SLAM2
{

// What pMap->GetAllMapPoints() returned, as pointers (to turn row entries back into MapPoint*) and resident in HBM.
struct HipMapSnapshot {
    vector<MapPoint *> vpPoints;
    std::shared_ptr<orbm_map> pMap;
};

HipMapSnapshot HipMapSnapshotOf(Map *pMap)
{
    HipMapSnapshot s;
    s.vpPoints = pMap->GetAllMapPoints();
    const size_t m = s.vpPoints.size();
    vector<float> pos(3 * m + 1), normal(3 * m + 1), minDistance(m + 1), maxDistance(m + 1);
    vector<uint8_t> desc(32 * m + 1);
    for (size_t i = 0; i < m; ++i) {
        MapPoint *pMP = s.vpPoints[i];
        const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), d = pMP->GetDescriptor();
        for (int k = 0; k < 3; ++k) { pos[3 * i + k] = P.at<float>(k); normal[3 * i + k] = Pn.at<float>(k); }
        minDistance[i] = pMP->GetMinDistanceInvariance();
        maxDistance[i] = pMP->GetMaxDistanceInvariance();
        memcpy(&desc[32 * i], d.ptr<uint8_t>(), 32);
    }
    orbm_map *h = NULL;
    if (orbm_map_create(pos.data(), normal.data(), minDistance.data(), maxDistance.data(), desc.data(), (int)m, &h) == ORBX_OK)
        s.pMap = std::shared_ptr<orbm_map>(h, [](orbm_map *p) { orbm_map_destroy(p); });
    return s;
}

static cv::Mat PoseOf(const double R[3][3], const double t[3])
{
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T.at<float>(i, j) = (float)R[i][j];
        T.at<float>(i, 3) = (float)t[i];
    }
    return T;
}

// The stage behind "Set storage for optional evaluation of the projection" (:479) up to the function's end, given what the
// histogram code in front of it left: the nBestPoses recorded poses with their inlier counts and the two thresholds.  nSlots =
// mvpMapPointMatches.size().  Returns what iterate returns from there on and sets vpMapPointMatches / vbInliers / nInliers /
// bNoMore as it does.
cv::Mat PnPsolverHipProjectBestPoses(Frame &rF, const HipMapSnapshot &snap, const double (*RPosesHist)[3][3], const double (*tPosesHist)[3],
                                     const int *inlierPosesHist, int nBestPoses, int max1histvalue, int max2histvalue, size_t nSlots,
                                     vector<MapPoint *> &vpMapPointMatches, vector<bool> &vbInliers, int &nInliers, bool &bNoMore)
{
    // the visits of the itHist / it walk, in its order; every pose that is visited is searched once
    const int bestHists[2] = {max1histvalue, max2histvalue};
    vector<int> visits, rowOf(nBestPoses > 0 ? nBestPoses : 1, -1);
    vector<double> R, t;
    for (int itHist = 0; itHist < 2; ++itHist)
        for (int it = 0; it < nBestPoses; ++it) {
            if (inlierPosesHist[it] < bestHists[itHist]) continue;
            if (rowOf[it] < 0) {
                rowOf[it] = (int)(t.size() / 3);
                for (int i = 0; i < 3; ++i) {
                    t.push_back(tPosesHist[it][i]);
                    for (int j = 0; j < 3; ++j) R.push_back(RPosesHist[it][i][j]);
                }
            }
            visits.push_back(it);
        }
    const int P = (int)(t.size() / 3), nFeatures = (int)rF.mvKeysUn.size();     // P <= 5: orbm_..._map_poses takes 16
    vector<int32_t> matched((size_t)P * nFeatures + 1, -1), nm(P + 1, 0);
    if (P > 0) {
        vector<uint8_t> has(nFeatures + 1, 0);
        for (int j = 0; j < nFeatures; ++j) has[j] = rF.mvpMapPoints[j] != NULL;
        const vector<int> b = rF.GetImageBounds();
        const orbm_camera cam = {Frame::fx, Frame::fy, Frame::cx, Frame::cy, b[0], b[1], b[2], b[3], Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY};
        if (!snap.pMap || orbm_frame_search_by_projection_map_poses(rF.mpHipFrame.get(), has.data(), snap.pMap.get(), R.data(), t.data(), P, &cam,
                                                                    rF.mvScaleFactors.data(), rF.mnScaleLevels, 15.0f, 0.75f, ORBmatcher::TH_RELOC,
                                                                    matched.data(), nm.data(), NULL) != ORBX_OK)
            visits.clear();     // no device, no result: as if no pose had been recorded
    }
    // the fold, in visiting order
    int bestVisit = -1, bestMatches = 0;
    for (size_t v = 0; v < visits.size(); ++v) {
        const int it = visits[v], row = rowOf[it], nMatched = nm[row];
        const int32_t *m = &matched[(size_t)row * nFeatures];
        if (nMatched > 30) {                    // (rows of later visits: speculative, dropped here)
            nInliers = nMatched;
            vbInliers = vector<bool>(nSlots, false);
            for (int j = 0; j < nFeatures; ++j)
                if (m[j] >= 0) { vbInliers[j] = true; vpMapPointMatches[j] = snap.vpPoints[m[j]]; }
            return PoseOf(RPosesHist[it], tPosesHist[it]);
        }
        if (bestVisit < 0 || nMatched > bestMatches) { bestVisit = (int)v; bestMatches = nMatched; }   // the first of the largest
    }
    if (bestVisit < 0) {
        bNoMore = true;
        return cv::Mat();
    }
    const int it = visits[bestVisit];
    const int32_t *m = &matched[(size_t)rowOf[it] * nFeatures];
    nInliers = bestMatches;
    vbInliers = vector<bool>(nSlots, false);
    for (int j = 0; j < nFeatures; ++j)
        if (m[j] >= 0) vbInliers[j] = true;    // (this return leaves vpMapPointMatches as it was, as the reference does)
    return PoseOf(RPosesHist[it], tPosesHist[it]);
}

} // namespace ORB_SLAM2
