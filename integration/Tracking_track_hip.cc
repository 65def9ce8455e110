// Tracking_track_hip.cc -- Tracking::TrackWithMotionModel (src/Tracking.cc:1222-1285) and Tracking::TrackLocalMap (:1287-1333) with
// their data planes as ONE library call each: the projection search chained into PoseOptimization on the device, one staged upload
// and one host wait per frame.  The walks over the pointer graph (MapPoint*: tests a device cannot make) and the
// bookkeeping on it stay here, in the reference's order.  Reference-side code: compiles in the ORB_SLAM2_E tree.  INTEGRATION.md 2:
// between UpdateLastFrame() and `if(mbOnlyTracking)` the body of TrackWithMotionModel becomes
//     int nmatches, nmatchesMap; if (!HipTrackWithMotionModel(...)) return false;
// and between UpdateLocalMap() and "Decide if the tracking was succesful" the body of TrackLocalMap becomes
//     mnMatchesInliers = HipTrackLocalMap(...).
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "hip_frame.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

static orbm_view TrackViewOf(const Frame &F)
{
    return orbm_view{Frame::fx, Frame::fy, Frame::cx, Frame::cy, F.mb, F.mbf, F.mfLogScaleFactor, F.mnScaleLevels, F.mvScaleFactors.data()};
}
static orbm_pose_camera TrackPoseCameraOf(const Frame &F)
{
    return orbm_pose_camera{Frame::fx, Frame::fy, Frame::cx, Frame::cy, F.mbf, (int32_t)F.mvInvLevelSigma2.size(), F.mvInvLevelSigma2.data()};
}

// Tracking.cc:1232-1276.  Tcw = mVelocity * mLastFrame.mTcw; th = 15 (7 for stereo, :1237-1241).  Returns false where the reference
// returns false at :1251-1252; else nmatches / nmatchesMap as the discard loop leaves them.
bool HipTrackWithMotionModel(Frame &CurrentFrame, const Frame &LastFrame, const cv::Mat &Tcw, int th, bool bMono, int &nmatches, int &nmatchesMap)
{
    CurrentFrame.SetPose(Tcw);                                                                  // :1232
    std::fill(CurrentFrame.mvpMapPoints.begin(), CurrentFrame.mvpMapPoints.end(), static_cast<MapPoint *>(NULL));   // :1234
    const int N = CurrentFrame.N;
    HipPointList last(LastFrame.N);
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);                              // Optimizer.cc:298 (the positions the solve reads)
        for (int i = 0; i < LastFrame.N; ++i) {
            MapPoint *pMP = LastFrame.mvpMapPoints[i];
            if (!pMP || LastFrame.mvbOutlier[i]) continue;                                      // ORBmatcher.cc:1555-1558
            last.set(i, pMP);
            last.octave[i] = LastFrame.mvKeys[i].octave;                                        // :1578
            last.angle[i] = LastFrame.mvKeysUn[i].angle;                                        // :1642
        }
    }
    float Tc[16], Tl[16], Tout[16];
    HipPose(CurrentFrame.mTcw, Tc); HipPose(LastFrame.mTcw, Tl);
    const orbm_view view = TrackViewOf(CurrentFrame);
    const orbm_pose_camera cam = TrackPoseCameraOf(CurrentFrame);
    const orbm_points pl = last.view();
    std::vector<int32_t> slot(N > 0 ? N : 1), chosen(LastFrame.N > 0 ? LastFrame.N : 1);
    std::vector<uint8_t> outlier(N > 0 ? N : 1, 0);
    orbm_track_result r;
    if (orbm_track_with_motion_model(CurrentFrame.mpHipFrame.get(), &view, &cam, Tc, Tl, &pl, (float)th, bMono, ORBmatcher::TH_HIGH,
                                     /*check_orientation=*/1, /*min_matches=*/20, slot.data(), chosen.data(), outlier.data(), Tout, &r,
                                     nullptr) != ORBX_OK)
        throw std::runtime_error(std::string("orbm_track_with_motion_model: ") + orbx_last_error());
    for (int j = 0; j < N; ++j)
        if (slot[j] >= 0) CurrentFrame.mvpMapPoints[j] = LastFrame.mvpMapPoints[slot[j]];       // ORBmatcher.cc:1634 (-2: :1664, already NULL)
    nmatches = r.nsearch; nmatchesMap = 0;
    if (!r.tracked) return false;                                                               // :1251-1252
    int nmp = 0;
    for (int j = 0; j < N; ++j)
        if (slot[j] >= 0) { CurrentFrame.mvbOutlier[j] = outlier[j] != 0; nmp++; }              // Optimizer.cc:312, :405-416
    if (nmp >= 3) CurrentFrame.SetPose(cv::Mat(4, 4, CV_32F, Tout).clone());                    // Optimizer.cc:385-386, :470-472
    for (int i = 0; i < N; i++) {                                                               // :1257-1276
        if (!CurrentFrame.mvpMapPoints[i] || !CurrentFrame.mvbOutlier[i]) continue;
        MapPoint *pMP = CurrentFrame.mvpMapPoints[i];
        CurrentFrame.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
        CurrentFrame.mvbOutlier[i] = false;
        pMP->mbTrackInView = false;
        pMP->mnLastFrameSeen = CurrentFrame.mnId;
    }
    nmatches = r.nmatches; nmatchesMap = r.nmatches_map;
    return true;
}

// Tracking.cc:1294-1320 behind UpdateLocalMap, with Tracking::SearchLocalPoints (:1335-1388) folded in.  th = 1, 3 with an RGB-D
// sensor, 5 shortly after a relocalisation (:1377-1383).  Returns mnMatchesInliers.
int HipTrackLocalMap(Frame &CurrentFrame, const std::vector<MapPoint *> &vpLocalMapPoints, int th, float nnratio, bool bOnlyTracking, bool bStereo)
{
    const int N = CurrentFrame.N;
    std::vector<uint8_t> baseHas(N > 0 ? N : 1, 0), baseTakes(N > 0 ? N : 1, 0), outlier(N > 0 ? N : 1, 0);
    std::vector<float> basePos(3 * (size_t)(N > 0 ? N : 1), 0.f);
    const size_t m = vpLocalMapPoints.size();
    HipPointList pts(m);
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);
        for (int j = 0; j < N; ++j) {                                                           // :1338-1355: do not search points already matched
            MapPoint *pMP = CurrentFrame.mvpMapPoints[j];
            if (!pMP) continue;
            if (pMP->isBad()) { CurrentFrame.mvpMapPoints[j] = static_cast<MapPoint *>(NULL); continue; }
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = CurrentFrame.mnId;
            pMP->mbTrackInView = false;
            baseHas[j] = 1; baseTakes[j] = pMP->Observations() > 0;
            const cv::Mat Xw = pMP->GetWorldPos();
            for (int k = 0; k < 3; ++k) basePos[3 * j + k] = Xw.at<float>(k);
        }
        for (size_t i = 0; i < m; ++i) {                                                        // :1359-1373
            MapPoint *pMP = vpLocalMapPoints[i];
            if (pMP->mnLastFrameSeen == CurrentFrame.mnId || pMP->isBad()) continue;
            pts.set(i, pMP);
        }
    }
    float Tc[16], Tout[16];
    HipPose(CurrentFrame.mTcw, Tc);
    const orbm_view view = TrackViewOf(CurrentFrame);
    const orbm_pose_camera cam = TrackPoseCameraOf(CurrentFrame);
    const orbm_points pl = pts.view();
    std::vector<int32_t> slot(N > 0 ? N : 1), chosen(m ? m : 1);
    std::vector<orbm_projected_point> proj(m ? m : 1);
    orbm_track_result r;
    if (orbm_track_local_map(CurrentFrame.mpHipFrame.get(), &view, &cam, Tc, &pl, baseHas.data(), basePos.data(), baseTakes.data(), (float)th,
                             0.5f, ORBmatcher::TH_HIGH, nnratio, slot.data(), chosen.data(), proj.data(), outlier.data(), Tout, &r,
                             nullptr) != ORBX_OK)
        throw std::runtime_error(std::string("orbm_track_local_map: ") + orbx_last_error());
    for (size_t i = 0; i < m; ++i) {                                                            // what isInFrustum leaves in the MapPoint (:1367-1371)
        if (!pts.valid[i]) continue;
        MapPoint *pMP = vpLocalMapPoints[i];
        pMP->mbTrackInView = proj[i].visible != 0;
        if (!proj[i].visible) continue;
        pMP->mTrackProjX = proj[i].u; pMP->mTrackProjY = proj[i].v; pMP->mTrackProjXR = proj[i].ur;
        pMP->mnTrackScaleLevel = proj[i].level; pMP->mTrackViewCos = proj[i].view_cos;
        pMP->IncreaseVisible();
    }
    int nmp = 0;
    for (int j = 0; j < N; ++j) {
        if (slot[j] >= 0) CurrentFrame.mvpMapPoints[j] = vpLocalMapPoints[slot[j]];             // ORBmatcher.cc:126
        if (CurrentFrame.mvpMapPoints[j]) { CurrentFrame.mvbOutlier[j] = outlier[j] != 0; nmp++; }   // Optimizer.cc:312, :405-416
    }
    if (nmp >= 3) CurrentFrame.SetPose(cv::Mat(4, 4, CV_32F, Tout).clone());                    // Optimizer.cc:385-386, :470-472
    for (int i = 0; i < N; i++) {                                                               // :1301-1320
        if (!CurrentFrame.mvpMapPoints[i]) continue;
        if (!CurrentFrame.mvbOutlier[i]) CurrentFrame.mvpMapPoints[i]->IncreaseFound();
        else if (bStereo) CurrentFrame.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
    }
    return bOnlyTracking ? r.nmatches : r.nmatches_map;
}

} // namespace ORB_SLAM2
