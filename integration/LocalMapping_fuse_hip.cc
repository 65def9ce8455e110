// integration/LocalMapping_fuse_hip.cc -- the two loops that call ORBmatcher::Fuse once per target keyframe over ONE list of map
// points, each as one library call for all (target, point) pairs plus one small call per refresh
// (orbslam_hip::ORBmatcher::FuseKeyFrames / FuseKeyFramesSim3 over orbm_fuse_keyframes):
//   HipFuseInTargets    LocalMapping::SearchInNeighbors   src/LocalMapping.cc:550-558    matcher.Fuse(pKFi, vpMapPointMatches)
//   HipSearchAndFuse    LoopClosing::SearchAndFuse        src/LoopClosing.cc:587-613     matcher.Fuse(pKF, cvScw, mvpLoopMapPoints, 4, vpReplacePoints)
//                                                                                        + the Replace loop behind it (:604-611)
// The shells keep the pointer graph: isBad(), IsInKeyFrame(), GetMapPoint(), Observations(), Replace(), AddObservation() /
// AddMapPoint(), GetMapPoints() run on the MapPoint* / KeyFrame* objects, in the reference's order, behind the device.
// MapPoint::Replace ends with ComputeDistinctiveDescriptors on the heir (src/MapPoint.cc:275): the library's loop reads
// GetDescriptor() of every heir after each target and computes the rows of the later targets again where the bytes changed.
// The reverse fuse of LocalMapping.cc:582 has one target and stays on ORBmatcher::Fuse.
//
// Written against the patched headers of reference.patch (KeyFrame::mpHipFrame, MapPoint's friend access); like the other shells
// it cannot be compiled where OpenCV is absent, and reference.patch does not carry it (its hunks are pinned).  The callers' loops
// are replaced by hand, see INTEGRATION.md section 2.
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "Converter.h"
#include "KeyFrame.h"
#include "LoopClosing.h"
#include "MapPoint.h"
#include "hip_frame.h"
#include "orbslam_hip.hpp"

namespace ORB_SLAM2
{

namespace
{
typedef orbslam_hip::ORBmatcher HipMatcher;
const size_t kMaxTargets = 128;       // targets per library loop; longer lists go in chunks, each chunk a loop of its own

// The target's pose and camera as ORBmatcher::Fuse reads them (src/ORBmatcher.cc:1028-1037).
HipMatcher::FuseTargetView TargetOf(KeyFrame *pKF, const float R[9], const float t[3], const float O[3])
{
    HipMatcher::FuseTargetView v;
    v.frame = pKF->mpHipFrame.get();
    std::copy(R, R + 9, v.pose.Rcw); std::copy(t, t + 3, v.pose.tcw); std::copy(O, O + 3, v.pose.Ow);
    const orbm_camera cam = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, 0, 0, 0, 0, (float)pKF->mnMinX, (float)pKF->mnMinY, (float)pKF->mnMaxX, (float)pKF->mnMaxY};
    v.pose.cam = cam;
    v.pose.mbf = pKF->mbf; v.pose.mfLogScaleFactor = pKF->mfLogScaleFactor;
    v.pose.mvScaleFactors = pKF->mvScaleFactors.data(); v.pose.mvInvLevelSigma2 = pKF->mvInvLevelSigma2.data();
    v.pose.mnScaleLevels = pKF->mnScaleLevels;
    return v;
}

// The pointer-graph side of the loop for the library's host logic (handles are MapPoint*).
struct FuseGraph {
    const std::vector<KeyFrame*> &targets;
    const std::vector<MapPoint*> &points;
    bool sim3;
    KeyFrame *pKF;
    std::set<MapPoint*> spAlreadyFound;
    std::vector<MapPoint*> vpReplacePoints;
    cv::Mat desc;                                   // keeps the bytes descriptor() handed out alive
    FuseGraph(const std::vector<KeyFrame*> &t, const std::vector<MapPoint*> &p, bool s) : targets(t), points(p), sim3(s), pKF(NULL) {}
    MapPoint *at(int i) const { return points[i]; }
    bool null(MapPoint *p) const { return !p; }
    bool isBad(MapPoint *p) const { return p->isBad(); }
    bool isInKeyFrame(MapPoint *p) const { return p->IsInKeyFrame(pKF); }
    bool alreadyFound(MapPoint *p) const { return spAlreadyFound.count(p) != 0; }
    MapPoint *slotOwner(int idx) const { return pKF->GetMapPoint(idx); }
    int observations(MapPoint *p) const { return p->Observations(); }
    void replace(MapPoint *dead, MapPoint *heir) { dead->Replace(heir); }
    void add(MapPoint *p, int idx) { p->AddObservation(pKF, idx); pKF->AddMapPoint(p, idx); }
    void recordReplace(int i, MapPoint *p) { vpReplacePoints[i] = p; }
    const uint8_t *descriptor(MapPoint *p) { desc = p->GetDescriptor(); return desc.ptr<uint8_t>(); }
    bool inTarget(MapPoint *p, int k) const { return sim3 ? targets[k]->GetMapPoints().count(p) != 0 : p->IsInKeyFrame(targets[k]); }
    void beginTarget(int k)
    {
        pKF = targets[k];
        if (sim3) {
            spAlreadyFound = pKF->GetMapPoints();                                   // ORBmatcher.cc:1194: a snapshot
            vpReplacePoints.assign(points.size(), static_cast<MapPoint*>(NULL));    // LoopClosing.cc:598
        }
    }
    template <class Report> void endTarget(int, Report report)
    {
        if (!sim3) return;
        for (size_t i = 0; i < points.size(); i++) {                                // LoopClosing.cc:604-611
            MapPoint *pRep = vpReplacePoints[i];
            if (pRep) { pRep->Replace(points[i]); report((int)i); }
        }
    }
};

// GetWorldPos / GetNormal / the distance range / GetDescriptor of every listed point, once per loop
void Flatten(const std::vector<MapPoint*> &points, HipPointList &pts, HipMatcher::MapPointArrays &mps)
{
    for (size_t i = 0; i < points.size(); ++i)
        if (points[i]) pts.set(i, points[i]);
    mps.pos = pts.pos.data(); mps.normal = pts.normal.data(); mps.mfMinDistance = pts.minDistance.data();
    mps.mfMaxDistance = pts.maxDistance.data(); mps.descriptors = pts.desc.data(); mps.n = (int)points.size();
}
}

// The forward loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:550-558): every matcher.Fuse(pKFi, vpMapPointMatches)
// over vpTargetKFs, th = 3.0 as the declaration's default.  vnFused[i] is what the reference's iteration i returns.  Returns false
// if the library refused a call (the map is then as far as the targets in front of the refused chunk took it).
bool HipFuseInTargets(const std::vector<KeyFrame*> &vpTargetKFs, const std::vector<MapPoint*> &vpMapPointMatches, std::vector<int> &vnFused,
                      const float th = 3.0)
{
    vnFused.clear();
    HipMatcher matcher;
    for (size_t k0 = 0; k0 < vpTargetKFs.size(); k0 += kMaxTargets) {
        const std::vector<KeyFrame*> chunk(vpTargetKFs.begin() + k0, vpTargetKFs.begin() + std::min(vpTargetKFs.size(), k0 + kMaxTargets));
        std::vector<HipMatcher::FuseTargetView> targets;
        for (size_t k = 0; k < chunk.size(); ++k) {
            KeyFrame *pKF = chunk[k];
            float Tcw[16], Rcw[9], tcw[3], Ow[3];
            HipPose(pKF->GetPose(), Tcw);
            const cv::Mat O = pKF->GetCameraCenter();
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rcw[3 * r + c] = Tcw[4 * r + c]; tcw[r] = Tcw[4 * r + 3]; Ow[r] = O.at<float>(r); }
            targets.push_back(TargetOf(pKF, Rcw, tcw, Ow));
        }
        HipPointList pts(vpMapPointMatches.size());
        HipMatcher::MapPointArrays mps;
        Flatten(vpMapPointMatches, pts, mps);        // (per chunk: the descriptors as they are when the chunk's loop begins)
        FuseGraph graph(chunk, vpMapPointMatches, false);
        const std::vector<int> n = matcher.FuseKeyFrames(targets, mps, th, graph);
        if (matcher.status() != ORBX_OK || n.size() != chunk.size()) return false;
        vnFused.insert(vnFused.end(), n.begin(), n.end());
    }
    return true;
}

// LoopClosing::SearchAndFuse (src/LoopClosing.cc:587-613) as a whole: for every corrected keyframe the Sim3 form of Fuse over
// mvpLoopMapPoints with th = 4 and the Replace loop behind it.  The map mutex of :602 is the caller's: take it around this call.
bool HipSearchAndFuse(const LoopClosing::KeyFrameAndPose &CorrectedPosesMap, const std::vector<MapPoint*> &mvpLoopMapPoints, const float th = 4.0)
{
    std::vector<KeyFrame*> all;
    std::vector<HipMatcher::FuseTargetView> views;
    for (LoopClosing::KeyFrameAndPose::const_iterator mit = CorrectedPosesMap.begin(), mend = CorrectedPosesMap.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        cv::Mat Scw = Converter::toCvMat(mit->second);
        cv::Mat sRcw = Scw.rowRange(0, 3).colRange(0, 3);                           // ORBmatcher.cc:1186-1192
        const float scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));
        cv::Mat Rcw = sRcw / scw;
        cv::Mat tcw = Scw.rowRange(0, 3).col(3) / scw;
        cv::Mat Ow = -Rcw.t() * tcw;
        float R[9], t[3], O[3];
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = Rcw.at<float>(r, c); t[r] = tcw.at<float>(r); O[r] = Ow.at<float>(r); }
        all.push_back(pKF); views.push_back(TargetOf(pKF, R, t, O));
    }
    HipMatcher matcher(0.8f);
    for (size_t k0 = 0; k0 < all.size(); k0 += kMaxTargets) {
        const size_t k1 = std::min(all.size(), k0 + kMaxTargets);
        const std::vector<KeyFrame*> chunk(all.begin() + k0, all.begin() + k1);
        const std::vector<HipMatcher::FuseTargetView> targets(views.begin() + k0, views.begin() + k1);
        HipPointList pts(mvpLoopMapPoints.size());
        HipMatcher::MapPointArrays mps;
        Flatten(mvpLoopMapPoints, pts, mps);
        FuseGraph graph(chunk, mvpLoopMapPoints, true);
        const std::vector<int> n = matcher.FuseKeyFramesSim3(targets, mps, th, graph);
        if (matcher.status() != ORBX_OK || n.size() != chunk.size()) return false;
    }
    return true;
}

} // namespace ORB_SLAM2
