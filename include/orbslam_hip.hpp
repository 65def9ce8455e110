// orbslam_hip.hpp -- C++ host classes over the C-ABI (header only).
//
// Same names, constructor arguments, getters and call semantics as the
// reference's classes (include/ORBextractor.h:46-112, include/ORBmatcher.h:37-111,
// Thirdparty/g2o/g2o/FEA/include/FEA2.h:94-304), with plain views instead of
// cv::Mat / std::vector<cv::KeyPoint> so the header needs no OpenCV.
// INTEGRATION.md shows the few lines that bind these to the cv:: signatures so
// that Tracking.cc / Frame.cc link unchanged.  Like the reference, nothing here
// throws; `status()` reports the last C-ABI status code.
#ifndef ORBSLAM_HIP_HPP
#define ORBSLAM_HIP_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "fem_hip.h"
#include "orbslam_hip.h"

namespace orbslam_hip {

// A CV_8UC1 image view: what cv::Mat::data / cols / rows / step carry.
struct ImageView {
    const uint8_t *data = nullptr;
    int cols = 0, rows = 0, step = 0;
    bool empty() const { return !data || cols <= 0 || rows <= 0; }
};

// One pyramid level on the host (mvImagePyramid[level]).
struct HostImage {
    std::vector<uint8_t> pixels;
    int cols = 0, rows = 0;
    ImageView view() const { return ImageView{pixels.data(), cols, rows, cols}; }
};

typedef orbx_keypoint KeyPoint; // 28-byte cv::KeyPoint layout

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 }; // ORBextractor.h:50

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
    {
        orbx_params p = {nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, /*blur_variant*/ 0, /*trig_variant*/ 0};
        mStatus = orbx_create(&p, &mHandle);
        if (mStatus == ORBX_OK) {
            mnLevels = nlevels;
            mvScaleFactor.resize(nlevels); mvInvScaleFactor.resize(nlevels);
            mvLevelSigma2.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
            orbx_get_scale_factors(mHandle, mvScaleFactor.data());
            orbx_get_inv_scale_factors(mHandle, mvInvScaleFactor.data());
            orbx_get_level_sigma2(mHandle, mvLevelSigma2.data());
            orbx_get_inv_level_sigma2(mHandle, mvInvLevelSigma2.data());
            mvImagePyramid.resize(nlevels);
        }
    }
    ~ORBextractor() { orbx_destroy(mHandle); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // Compute the ORB features and descriptors on an image; the mask is ignored
    // (ORBextractor.cc:1051-1113).  descriptors: n rows of 32 bytes.
    void operator()(const ImageView &image, const ImageView & /*mask*/, std::vector<KeyPoint> &keypoints,
                    std::vector<uint8_t> &descriptors)
    {
        if (image.empty()) return; // :1054-1055: outputs untouched
        mStatus = orbx_reserve(mHandle, image.cols, image.rows, 1);   // the capacity depends on the frame's aspect ratio (tiny quotas)
        if (mStatus != ORBX_OK) { keypoints.clear(); descriptors.clear(); return; }
        const int cap = orbx_keypoint_capacity(mHandle);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        mStatus = orbx_extract(mHandle, image.data, image.cols, image.rows, image.step, keypoints.data(),
                               descriptors.data(), cap, &n);
        if (mStatus != ORBX_OK) n = 0;
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32); // n == 0: descriptors.release() (:1072-1073)
        mPyramidStale = true;
    }

    void MarkPyramidStale() { mPyramidStale = true; }   // after a call that extracted through the handle (ExtractPair)
    int GetLevels() const { return mnLevels; }
    float GetScaleFactor() const { return mnLevels > 1 ? mvScaleFactor[1] : 1.0f; }
    std::vector<float> GetScaleFactors() const { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() const { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() const { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2; }

    // Public in the reference (ORBextractor.h:86) and read by
    // Frame::ComputeStereoMatches: call SyncImagePyramid() before reading it.
    std::vector<HostImage> mvImagePyramid;
    void SyncImagePyramid()
    {
        if (!mPyramidStale) return;
        for (int l = 0; l < mnLevels; ++l) {
            int w = 0, h = 0;
            if (orbx_level_size(mHandle, l, &w, &h) != ORBX_OK) return;
            HostImage &im = mvImagePyramid[l];
            im.cols = w; im.rows = h; im.pixels.resize((size_t)w * h);
            mStatus = orbx_pyramid_level(mHandle, 0, l, im.pixels.data(), w);
        }
        mPyramidStale = false;
    }

    int status() const { return mStatus; }
    orbx_extractor *handle() { return mHandle; }

private:
    orbx_extractor *mHandle = nullptr;
    int mnLevels = 0, mStatus = ORBX_OK;
    bool mPyramidStale = true;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// The two ExtractORB calls of a stereo frame (Frame.cc:78-81: two threads, then join) from one thread: both images' kernel chains
// are enqueued before the host waits for either (orbx_extract_pair).  Outputs as from left(...) and right(...).
inline int ExtractPair(ORBextractor &left, const ImageView &image_left, std::vector<KeyPoint> &keys_left, std::vector<uint8_t> &desc_left,
                       ORBextractor &right, const ImageView &image_right, std::vector<KeyPoint> &keys_right, std::vector<uint8_t> &desc_right)
{
    if (image_left.empty() || image_right.empty() || image_left.cols != image_right.cols || image_left.rows != image_right.rows ||
        image_left.step != image_right.step)
        return ORBX_ERR_ARG;
    int rc = orbx_reserve(left.handle(), image_left.cols, image_left.rows, 1);
    if (rc == ORBX_OK) rc = orbx_reserve(right.handle(), image_right.cols, image_right.rows, 1);
    if (rc != ORBX_OK) return rc;
    const int capl = orbx_keypoint_capacity(left.handle()), capr = orbx_keypoint_capacity(right.handle());
    keys_left.resize(capl); desc_left.resize((size_t)capl * 32); keys_right.resize(capr); desc_right.resize((size_t)capr * 32);
    int nl = 0, nr = 0;
    rc = orbx_extract_pair(left.handle(), image_left.data, right.handle(), image_right.data, image_left.cols, image_left.rows, image_left.step,
                           keys_left.data(), desc_left.data(), capl, &nl, keys_right.data(), desc_right.data(), capr, &nr);
    if (rc != ORBX_OK) nl = nr = 0;
    keys_left.resize(nl); desc_left.resize((size_t)nl * 32); keys_right.resize(nr); desc_right.resize((size_t)nr * 32);
    left.MarkPyramidStale(); right.MarkPyramidStale();
    return rc;
}

// Frame::ComputeStereoMatches (src/Frame.cc:527-701) on the results the two
// extractors still hold on the device after operator() ran on the left / right image.
inline int ComputeStereoMatches(ORBextractor &left, ORBextractor &right, float mb, float mbf,
                                std::vector<float> &mvuRight, std::vector<float> &mvDepth)
{
    const int cap = orbx_keypoint_capacity(left.handle());
    mvuRight.assign(cap, -1.0f);
    mvDepth.assign(cap, -1.0f);
    int n = 0;
    int rc = orbx_stereo_match(left.handle(), right.handle(), mb, mbf, nullptr);
    if (rc == ORBX_OK) rc = orbx_stereo_download(left.handle(), 0, mvuRight.data(), mvDepth.data(), cap, &n);
    mvuRight.resize(rc == ORBX_OK ? n : 0);
    mvDepth.resize(rc == ORBX_OK ? n : 0);
    return rc;
}

namespace DBoW2 {
typedef std::map<unsigned int, double> BowVector;                          // DBoW2/BowVector.h:57
typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;    // DBoW2/FeatureVector.h:23
}

class ORBmatcher {
public:
    static const int TH_LOW = 45, TH_HIGH = 95, TH_RELOC = 60, HISTO_LENGTH = 30; // ORBmatcher.cc:37-40

    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    // ORBmatcher::DescriptorDistance(a, b), a/b = 32-byte rows.
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b)
    {
        uint16_t d = 0;
        return orbm_hamming_matrix(a, 1, b, 1, &d) == ORBX_OK ? (int)d : -1;
    }

    // The selection loop of every Search* function over gated candidates
    // (candidate order = GetFeaturesInArea / BoW-member order), then the
    // acceptance test bestDist<=th && bestDist<bestDist2*mfNNratio.
    // Returns the number of accepted matches; vnMatches12[i] = index in B or -1.
    int MatchCandidates(const uint8_t *A, int nA, const uint8_t *B, int nB, const std::vector<int32_t> &candOff,
                        const std::vector<int32_t> &candIdx, int th, std::vector<int32_t> &vnMatches12,
                        std::vector<int32_t> *bestDist = nullptr)
    {
        std::vector<int32_t> best(nA), second(nA), idx(nA);
        vnMatches12.assign(nA, -1);
        if (orbm_match_candidates(A, nA, B, nB, candOff.data(), candIdx.data(), best.data(), second.data(), idx.data()) != ORBX_OK)
            return 0;
        int n = 0;
        orbm_match_filter(nA, best.data(), second.data(), idx.data(), th, mfNNratio, vnMatches12.data(), &n);
        if (bestDist) *bestDist = best;
        return n;
    }

    // Which kernel MatchBruteForce (and orbm_match_batch_dev) launch: ORBM_ALLPAIRS_AUTO / _POPCOUNT / _MFMA; same results.
    static int SetAllPairsKernel(int kind) { return orbm_set_allpairs_kernel(kind); }

    int MatchBruteForce(const uint8_t *A, int nA, const uint8_t *B, int nB, int th, std::vector<int32_t> &vnMatches12)
    {
        std::vector<int32_t> best(nA), second(nA), idx(nA);
        vnMatches12.assign(nA, -1);
        if (orbm_match_bruteforce(A, nA, B, nB, best.data(), second.data(), idx.data()) != ORBX_OK) return 0;
        int n = 0;
        orbm_match_filter(nA, best.data(), second.data(), idx.data(), th, mfNNratio, vnMatches12.data(), &n);
        return n;
    }

    // What the whole-loop searches read of a Frame / KeyFrame (src/Frame.h): mvKeysUn, mDescriptors (N x 32),
    // mvuRight (may be null: monocular), the grid bounds mnMinX..mnMaxY.
    struct FrameView {
        const orbx_keypoint *mvKeysUn = nullptr;
        const uint8_t *mDescriptors = nullptr;
        int N = 0;
        const float *mvuRight = nullptr;
        float mnMinX = 0.f, mnMinY = 0.f, mnMaxX = 0.f, mnMaxY = 0.f;
    };
    // One projected map point of the SearchByProjection loops: window (u, v, r), level range, xr = u - bf/z,
    // MapPoint::GetDescriptor(), the angle of its source keypoint, and whether the pointer it leaves in
    // mvpMapPoints makes later points skip that keypoint (Observations() > 0, or always).
    struct ProjectedPoint {
        orbm_window_query window;
        const uint8_t *descriptor;
        float angle;
        bool blocksSlot;
    };

    // ORBmatcher::SearchByProjection loops (ORBmatcher.cc:46-132, :491-604, :1529-1671, :1673-1800) over points
    // the caller has projected, in the caller's order.  occupied[j]: keypoint j is skipped from the start.
    // slotOwner[j] = point that ends in mvpMapPoints[j] (-1 untouched, -2 set to NULL by the rotation check).
    int SearchByProjection(const FrameView &F, const std::vector<ProjectedPoint> &points, const std::vector<uint8_t> &occupied,
                           int thAccept, bool ratioOnSameLevel, std::vector<int32_t> &slotOwner)
    {
        const int nq = (int)points.size();
        std::vector<orbm_window_query> q(nq);
        std::vector<uint8_t> qd((size_t)32 * nq), tk(nq);
        std::vector<float> qa(nq);
        for (int i = 0; i < nq; ++i) {
            q[i] = points[i].window; qa[i] = points[i].angle; tk[i] = points[i].blocksSlot;
            std::copy(points[i].descriptor, points[i].descriptor + 32, &qd[(size_t)32 * i]);
        }
        slotOwner.assign(F.N, -1);
        std::vector<int32_t> mq(nq);
        int nm = 0;
        mStatus = orbm_search_projection(q.data(), qd.data(), qa.data(), tk.data(), nq, F.mvKeysUn, F.mDescriptors, F.N,
                                         occupied.empty() ? nullptr : occupied.data(), F.mvuRight, F.mnMinX, F.mnMinY, F.mnMaxX,
                                         F.mnMaxY, thAccept, mfNNratio, ratioOnSameLevel, mbCheckOrientation, slotOwner.data(),
                                         mq.data(), &nm);
        return mStatus == ORBX_OK ? nm : 0;
    }

    // ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:606-721);
    // vbPrevMatched as x0, y0, x1, y1, ...
    int SearchForInitialization(const FrameView &F1, const FrameView &F2, std::vector<float> &vbPrevMatched,
                                std::vector<int32_t> &vnMatches12, int windowSize = 10)
    {
        vnMatches12.assign(F1.N, -1);
        int nm = 0;
        mStatus = orbm_search_for_initialization(F1.mvKeysUn, F1.mDescriptors, F1.N, F2.mvKeysUn, F2.mDescriptors, F2.N,
                                                 vbPrevMatched.data(), F2.mnMinX, F2.mnMinY, F2.mnMaxX, F2.mnMaxY, windowSize,
                                                 mfNNratio, mbCheckOrientation, vnMatches12.data(), &nm);
        return mStatus == ORBX_OK ? nm : 0;
    }

    // Candidate loop of ORBmatcher::Fuse (ORBmatcher.cc:1092-1146): best keypoint per projected map point under the
    // reprojection-error gate; invLevelSigma2 == nullptr: no gate (the Sim3 form).  The map update stays with the caller.
    int FuseCandidates(const FrameView &KF, const std::vector<ProjectedPoint> &points, const float *invLevelSigma2, int nLevels,
                       std::vector<int32_t> &bestDist, std::vector<int32_t> &bestIdx)
    {
        const int nq = (int)points.size();
        std::vector<orbm_window_query> q(nq);
        std::vector<uint8_t> qd((size_t)32 * nq);
        for (int i = 0; i < nq; ++i) { q[i] = points[i].window; std::copy(points[i].descriptor, points[i].descriptor + 32, &qd[(size_t)32 * i]); }
        bestDist.assign(nq, 256); bestIdx.assign(nq, -1);
        mStatus = orbm_search_fuse(q.data(), qd.data(), nq, KF.mvKeysUn, KF.mDescriptors, KF.N, KF.mvuRight, invLevelSigma2, nLevels,
                                   KF.mnMinX, KF.mnMinY, KF.mnMaxX, KF.mnMaxY, bestDist.data(), bestIdx.data());
        return mStatus;
    }

    // What the projection kernels read of a Frame / KeyFrame pose (src/Frame.cc:270-282, KeyFrame::GetRotation ...):
    // mRcw (row-major), mtcw, mOw as the float cv::Mat members hold them, the intrinsics, the grid bounds
    // mnMinX .. mnMaxY (in cam.grid_*), mbf, mfLogScaleFactor, mvScaleFactors.
    struct PoseView {
        float Rcw[9], tcw[3], Ow[3];
        orbm_camera cam;
        float mbf = 0.f, mfLogScaleFactor = 0.f;
        const float *mvScaleFactors = nullptr;
        const float *mvInvLevelSigma2 = nullptr;
        int mnScaleLevels = 0;
    };
    // Map points gathered by the caller from a vector<MapPoint*>: GetWorldPos(), GetNormal(), mfMinDistance,
    // mfMaxDistance, GetDescriptor(), one entry per list position (entries of NULL pointers are never read back).
    struct MapPointArrays {
        const float *pos = nullptr, *normal = nullptr, *mfMinDistance = nullptr, *mfMaxDistance = nullptr;
        const uint8_t *descriptors = nullptr;
        int n = 0;
    };

    // Frame::isInFrustum + MapPoint::PredictScale for all points at once (Frame.cc:284-340, MapPoint.cc:464-480):
    // out[i] = {mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos, dist, mnTrackScaleLevel, mbTrackInView}, windows[i] =
    // the GetFeaturesInArea query of SearchByProjection(Frame&, vector<MapPoint*>&, th) (ORBmatcher.cc:62-70).
    int ProjectInFrustum(const PoseView &F, const MapPointArrays &mps, float viewingCosLimit, float th,
                         std::vector<orbm_projected_point> &out, std::vector<orbm_window_query> &windows)
    {
        out.resize(mps.n); windows.resize(mps.n);
        mStatus = orbm_project_points(ORBM_PROJECT_FRUSTUM, mps.pos, mps.normal, mps.mfMinDistance, mps.mfMaxDistance, mps.n, F.Rcw,
                                      F.tcw, F.Ow, &F.cam, F.mbf, viewingCosLimit, F.mfLogScaleFactor, F.mvScaleFactors,
                                      F.mnScaleLevels, th, out.data(), windows.data());
        return mStatus;
    }

    // ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) as a whole (ORBmatcher.cc:1026-1176): projection of every
    // listed point (:1053-1094) and the gated candidate loop (:1092-1146) on the device, then the loop's skips (:1046-1053)
    // and its map update (:1149-1170) on the host in the list's order -- the candidate search of a point does not depend
    // on the map state, the skips and the update do.  `map` supplies the pointer-graph side through handles H (e.g.
    // MapPoint*): H at(int i) (vpMapPoints[i], a null handle for NULL), bool null(H), bool isBad(H), bool
    // isInKeyFrame(H), H slotOwner(int idx) (pKF->GetMapPoint), int observations(H), void replace(H dead, H heir)
    // (dead->Replace(heir)), void add(H, int idx) (AddObservation + AddMapPoint).
    template <class MapOps>
    int Fuse(const FrameView &KF, const PoseView &pose, const MapPointArrays &mps, float th, MapOps &map)
    {
        std::vector<orbm_projected_point> proj;
        std::vector<int32_t> best, idx;
        if (fuseCandidates(KF, pose, mps, th, false, proj, best, idx) != ORBX_OK) return 0;
        return fuseReplay(proj, best, idx, map);
    }
    // ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th, vpReplacePoint) (ORBmatcher.cc:1178-1301):
    // pose = the Sim3 decomposed as :1188-1192 do; `map` needs at / null / isBad / slotOwner / add as above, plus
    // bool alreadyFound(H) (spAlreadyFound.count(pMP): the SNAPSHOT of pKF->GetMapPoints() from before the call) and
    // void recordReplace(int i, H) (vpReplacePoint[i] = pMPinKF); it never replaces.
    template <class MapOps>
    int FuseSim3(const FrameView &KF, const PoseView &pose, const MapPointArrays &mps, float th, MapOps &map)
    {
        std::vector<orbm_projected_point> proj;
        std::vector<int32_t> best, idx;
        if (fuseCandidates(KF, pose, mps, th, true, proj, best, idx) != ORBX_OK) return 0;
        return fuseReplaySim3(proj, best, idx, map);
    }
    int fuseCandidates(const FrameView &KF, const PoseView &pose, const MapPointArrays &mps, float th, bool sim3,
                       std::vector<orbm_projected_point> &proj, std::vector<int32_t> &best, std::vector<int32_t> &idx)
    {
        proj.resize(mps.n);
        std::vector<orbm_window_query> q(mps.n);
        mStatus = orbm_project_points(sim3 ? ORBM_PROJECT_FUSE_SIM3 : ORBM_PROJECT_FUSE, mps.pos, mps.normal, mps.mfMinDistance,
                                      mps.mfMaxDistance, mps.n, pose.Rcw, pose.tcw, pose.Ow, &pose.cam, pose.mbf, 0.f,
                                      pose.mfLogScaleFactor, pose.mvScaleFactors, pose.mnScaleLevels, th, proj.data(), q.data());
        if (mStatus != ORBX_OK) return mStatus;
        best.assign(mps.n, 256); idx.assign(mps.n, -1);
        mStatus = orbm_search_fuse(q.data(), mps.descriptors, mps.n, KF.mvKeysUn, KF.mDescriptors, KF.N, KF.mvuRight,
                                   sim3 ? nullptr : pose.mvInvLevelSigma2, pose.mnScaleLevels, KF.mnMinX, KF.mnMinY, KF.mnMaxX,
                                   KF.mnMaxY, best.data(), idx.data());
        return mStatus;
    }

    // Tail of the Fuse loop, ORBmatcher.cc:1046-1053 and :1149-1170, in list order.
    template <class MapOps>
    static int fuseReplay(const std::vector<orbm_projected_point> &proj, const std::vector<int32_t> &best,
                          const std::vector<int32_t> &idx, MapOps &map)
    {
        int nFused = 0;
        for (int i = 0; i < (int)proj.size(); ++i) {
            auto pMP = map.at(i);
            if (map.null(pMP)) continue;
            if (map.isBad(pMP) || map.isInKeyFrame(pMP)) continue;
            if (!proj[i].visible || idx[i] < 0) continue;      // projection tests failed / vIndices.empty() / no candidate
            if (best[i] <= TH_LOW) {
                auto pMPinKF = map.slotOwner(idx[i]);
                if (!map.null(pMPinKF)) {
                    if (!map.isBad(pMPinKF)) {
                        if (map.observations(pMPinKF) > map.observations(pMP)) map.replace(pMP, pMPinKF);
                        else map.replace(pMPinKF, pMP);
                    }
                } else {
                    map.add(pMP, idx[i]);
                }
                ++nFused;
            }
        }
        return nFused;
    }

    // Tail of the Sim3 form, ORBmatcher.cc:1194-1205 and :1279-1296: the skips read spAlreadyFound, a snapshot of
    // pKF->GetMapPoints() taken before the loop -- map.alreadyFound(H) must answer from that snapshot, not from the
    // state the loop is changing (a point the loop adds is processed again when the list repeats it); a taken slot is
    // only recorded (vpReplacePoint[iMP] = pMPinKF: map.recordReplace(i, pMPinKF)), a free one gets the point.
    template <class MapOps>
    static int fuseReplaySim3(const std::vector<orbm_projected_point> &proj, const std::vector<int32_t> &best,
                              const std::vector<int32_t> &idx, MapOps &map)
    {
        int nFused = 0;
        for (int i = 0; i < (int)proj.size(); ++i) {
            auto pMP = map.at(i);
            if (map.null(pMP) || map.isBad(pMP) || map.alreadyFound(pMP)) continue;
            if (!proj[i].visible || idx[i] < 0) continue;
            if (best[i] <= TH_LOW) {
                auto pMPinKF = map.slotOwner(idx[i]);
                if (!map.null(pMPinKF)) { if (!map.isBad(pMPinKF)) map.recordReplace(i, pMPinKF); }
                else map.add(pMP, idx[i]);
                ++nFused;
            }
        }
        return nFused;
    }

    // The loop `for pKFi in targets: matcher.Fuse(pKFi, vpMapPointMatches)` of LocalMapping::SearchInNeighbors
    // (LocalMapping.cc:550-558) as a whole: ONE orbm_fuse_keyframes call for all K x m pairs, then fuseReplay target by target
    // in list order.  MapPoint::Replace ends with ComputeDistinctiveDescriptors on the heir (MapPoint.cc:275), so a list
    // entry's descriptor can change between two targets: after target k the rows of the LATER targets are computed again, in
    // one more call, for the entries whose handle a replace named as the heir, that are not bad and whose map.descriptor(H)
    // differs bytewise from the bytes their rows were computed with.  The result is the sequential loop's; host waits = 1 +
    // refreshes (LastFuseKeyFramesWaits / LastFuseKeyFramesRefreshes).  One pyramid (targets[0].pose) serves all targets.
    // `map`: what fuseReplay asks for, answered for the CURRENT target, plus void beginTarget(int k), void endTarget(int k,
    // report) (report(int i): the caller replaced into list entry i; the plain form has nothing to report), const uint8_t
    // *descriptor(H) (32 bytes) and, for the mask, bool inTarget(H, int k) (pMP->IsInKeyFrame(target k) now).  The mask is an
    // optimisation only: the tail tests every skip again at its own time.  Handles must be usable as std::map keys.
    struct FuseTargetView {
        const orbm_frame *frame = nullptr;      // the keyframe, resident
        PoseView pose;                          // Sim3 form: Rcw = sRcw / s, tcw = t / s, Ow = -Rcw' tcw (ORBmatcher.cc:1188-1192)
    };
    template <class MapOps>
    std::vector<int> FuseKeyFrames(const std::vector<FuseTargetView> &targets, const MapPointArrays &mps, float th, MapOps &map)
    {
        DeviceFuseCandidates cand{this, &mps, th, false};
        return fuseKeyFramesWith(cand, targets, mps, false, map);
    }
    // The loop of LoopClosing::SearchAndFuse (LoopClosing.cc:587-613) over the Sim3 form: beginTarget(k) takes the
    // spAlreadyFound snapshot of target k, endTarget(k, report) runs the caller's Replace loop (:604-611) and reports every
    // list index it replaced into; inTarget(H, k): H is among target k's map points now.
    template <class MapOps>
    std::vector<int> FuseKeyFramesSim3(const std::vector<FuseTargetView> &targets, const MapPointArrays &mps, float th, MapOps &map)
    {
        DeviceFuseCandidates cand{this, &mps, th, true};
        return fuseKeyFramesWith(cand, targets, mps, true, map);
    }
    int LastFuseKeyFramesWaits() const { return mFuseKeyFramesWaits; }
    int LastFuseKeyFramesRefreshes() const { return mFuseKeyFramesRefreshes; }

    // The candidate stage of FuseKeyFrames on the device: rows [K][points.size()] for the list entries `points` with the
    // descriptors `desc` (32 bytes each, in that order) and the mask `active`.  Returns the host waits of the call, -1 on error.
    struct DeviceFuseCandidates {
        ORBmatcher *self; const MapPointArrays *mps; float th; bool sim3;
        int operator()(const FuseTargetView *targets, int K, const std::vector<int> &points, const uint8_t *desc, const uint8_t *active,
                       int32_t *best, int32_t *idx, orbm_projected_point *proj) const
        {
            const int m = (int)points.size();
            std::vector<orbm_fuse_target> t((size_t)K);
            for (int k = 0; k < K; ++k) {
                t[k].frame = targets[k].frame;
                std::copy(targets[k].pose.Rcw, targets[k].pose.Rcw + 9, t[k].Rcw);
                std::copy(targets[k].pose.tcw, targets[k].pose.tcw + 3, t[k].tcw);
                std::copy(targets[k].pose.Ow, targets[k].pose.Ow + 3, t[k].Ow);
                t[k].cam = targets[k].pose.cam; t[k].mbf = targets[k].pose.mbf;
            }
            std::vector<float> pos((size_t)3 * m), nrm((size_t)3 * m), mn(m), mx(m);
            for (int j = 0; j < m; ++j) {
                const int i = points[j];
                std::copy(mps->pos + 3 * i, mps->pos + 3 * i + 3, &pos[(size_t)3 * j]);
                std::copy(mps->normal + 3 * i, mps->normal + 3 * i + 3, &nrm[(size_t)3 * j]);
                mn[j] = mps->mfMinDistance[i]; mx[j] = mps->mfMaxDistance[i];
            }
            const PoseView &p0 = targets[0].pose;
            self->mStatus = orbm_fuse_keyframes(t.data(), K, sim3, pos.data(), nrm.data(), mn.data(), mx.data(), desc, m, active, th,
                                                p0.mfLogScaleFactor, p0.mvScaleFactors, sim3 ? nullptr : p0.mvInvLevelSigma2,
                                                p0.mnScaleLevels, best, idx, proj);
            return self->mStatus == ORBX_OK ? orbm_debug_last_fuse_keyframes_waits() : -1;
        }
    };

    // FuseKeyFrames / FuseKeyFramesSim3 over any candidate stage (the tests put a stub in the device's place).
    template <class Candidates, class MapOps>
    std::vector<int> fuseKeyFramesWith(Candidates &cand, const std::vector<FuseTargetView> &targets, const MapPointArrays &mps, bool sim3,
                                       MapOps &map)
    {
        const int K = (int)targets.size(), m = mps.n;
        mFuseKeyFramesWaits = 0; mFuseKeyFramesRefreshes = 0;
        std::vector<int> nFused;
        if (K == 0) return nFused;
        typedef decltype(map.at(0)) H;
        std::vector<uint8_t> desc(mps.descriptors, mps.descriptors + (size_t)32 * m);    // the bytes the rows were computed with
        // mask from the map state at entry; handle -> list indices (the list holds duplicates and NULL entries)
        std::vector<uint8_t> active((size_t)K * m, 0);
        std::map<H, std::vector<int>> where;
        std::vector<int> all(m);
        for (int i = 0; i < m; ++i) {
            all[i] = i;
            H h = map.at(i);
            if (map.null(h)) continue;
            where[h].push_back(i);
            if (map.isBad(h)) continue;
            for (int k = 0; k < K; ++k) active[(size_t)k * m + i] = !map.inTarget(h, k);
        }
        std::vector<int32_t> best((size_t)K * m, 256), idx((size_t)K * m, -1);
        std::vector<orbm_projected_point> proj((size_t)K * m);
        int w = cand(targets.data(), K, all, desc.data(), active.data(), best.data(), idx.data(), proj.data());
        if (w < 0) return nFused;
        mFuseKeyFramesWaits += w;
        std::vector<char> heir(m);
        for (int k = 0; k < K; ++k) {
            std::fill(heir.begin(), heir.end(), 0);
            auto mark = [&](const H &h) {
                auto it = where.find(h);
                if (it != where.end()) for (int i : it->second) heir[i] = 1;
            };
            auto report = [&](int i) { if (i >= 0 && i < m && !map.null(map.at(i))) mark(map.at(i)); };
            map.beginTarget(k);
            FuseHeirLog<MapOps, decltype(mark)> tail{map, mark};
            const std::vector<orbm_projected_point> prow(proj.begin() + (size_t)k * m, proj.begin() + (size_t)(k + 1) * m);
            const std::vector<int32_t> brow(best.begin() + (size_t)k * m, best.begin() + (size_t)(k + 1) * m),
                                       irow(idx.begin() + (size_t)k * m, idx.begin() + (size_t)(k + 1) * m);
            nFused.push_back(sim3 ? fuseReplaySim3(prow, brow, irow, tail) : fuseReplay(prow, brow, irow, tail));
            map.endTarget(k, report);
            std::vector<int> dirty;
            for (int i = 0; i < m; ++i) {
                if (!heir[i]) continue;
                H h = map.at(i);
                if (map.isBad(h)) continue;
                const uint8_t *d = map.descriptor(h);
                if (!std::equal(d, d + 32, &desc[(size_t)32 * i])) { std::copy(d, d + 32, &desc[(size_t)32 * i]); dirty.push_back(i); }
            }
            if (dirty.empty() || k + 1 >= K) continue;
            const int nd = (int)dirty.size(), Kr = K - k - 1;
            std::vector<uint8_t> d2((size_t)32 * nd), a2((size_t)Kr * nd);
            std::vector<int32_t> b2((size_t)Kr * nd, 256), i2((size_t)Kr * nd, -1);
            std::vector<orbm_projected_point> p2((size_t)Kr * nd);
            for (int j = 0; j < nd; ++j) {
                std::copy(&desc[(size_t)32 * dirty[j]], &desc[(size_t)32 * dirty[j]] + 32, &d2[(size_t)32 * j]);
                for (int r = 0; r < Kr; ++r) a2[(size_t)r * nd + j] = active[(size_t)(k + 1 + r) * m + dirty[j]];
            }
            w = cand(targets.data() + k + 1, Kr, dirty, d2.data(), a2.data(), b2.data(), i2.data(), p2.data());
            if (w < 0) return nFused;
            mFuseKeyFramesWaits += w; ++mFuseKeyFramesRefreshes;
            for (int r = 0; r < Kr; ++r)
                for (int j = 0; j < nd; ++j) {
                    const size_t o = (size_t)(k + 1 + r) * m + dirty[j];
                    best[o] = b2[(size_t)r * nd + j]; idx[o] = i2[(size_t)r * nd + j]; proj[o] = p2[(size_t)r * nd + j];
                }
        }
        return nFused;
    }
    // `map` as the Fuse tails see it, marking the heir of every replace(dead, heir).
    template <class MapOps, class Mark>
    struct FuseHeirLog {
        MapOps &map; Mark &mark;
        auto at(int i) -> decltype(map.at(i)) { return map.at(i); }
        template <class H> bool null(const H &h) { return map.null(h); }
        template <class H> bool isBad(const H &h) { return map.isBad(h); }
        template <class H> bool isInKeyFrame(const H &h) { return map.isInKeyFrame(h); }
        template <class H> bool alreadyFound(const H &h) { return map.alreadyFound(h); }
        auto slotOwner(int idx) -> decltype(map.slotOwner(idx)) { return map.slotOwner(idx); }
        template <class H> int observations(const H &h) { return map.observations(h); }
        template <class H> void replace(const H &dead, const H &heir) { map.replace(dead, heir); mark(heir); }
        template <class H> void add(const H &h, int idx) { map.add(h, idx); }
        template <class H> void recordReplace(int i, const H &h) { map.recordReplace(i, h); }
    };

    // ORBmatcher::SearchBySim3 (ORBmatcher.cc:1303-1527) over projected points: points12[i1] = map point i1 of KF1 seen
    // in KF2 (window.r < 0: skipped), points21 the other way; levels [l-1, l], <= TH_HIGH, then the agreement check.
    int SearchBySim3(const FrameView &KF1, const FrameView &KF2, const std::vector<ProjectedPoint> &points12,
                     const std::vector<ProjectedPoint> &points21, std::vector<int32_t> &vnMatches12)
    {
        auto one_way = [&](const FrameView &dst, const std::vector<ProjectedPoint> &pts, std::vector<int32_t> &m) {
            const int nq = (int)pts.size();
            std::vector<orbm_window_query> q(nq);
            std::vector<uint8_t> qd((size_t)32 * nq);
            for (int i = 0; i < nq; ++i) { q[i] = pts[i].window; std::copy(pts[i].descriptor, pts[i].descriptor + 32, &qd[(size_t)32 * i]); }
            std::vector<int32_t> best(nq), bl(nq), second(nq), sl(nq), idx(nq);
            mStatus = orbm_search_window(q.data(), qd.data(), nq, dst.mvKeysUn, dst.mDescriptors, dst.N, nullptr, nullptr, dst.mnMinX,
                                         dst.mnMinY, dst.mnMaxX, dst.mnMaxY, INT32_MAX, best.data(), bl.data(), second.data(), sl.data(),
                                         idx.data());
            m.assign(nq, -1);
            for (int i = 0; i < nq && mStatus == ORBX_OK; ++i)
                if (idx[i] >= 0 && best[i] <= TH_HIGH) m[i] = idx[i];
        };
        std::vector<int32_t> m1, m2;
        one_way(KF2, points12, m1);
        if (mStatus == ORBX_OK) one_way(KF1, points21, m2);
        vnMatches12.assign(points12.size(), -1);
        int nFound = 0;
        for (size_t i1 = 0; i1 < m1.size() && mStatus == ORBX_OK; ++i1)
            if (m1[i1] >= 0 && m1[i1] < (int32_t)m2.size() && m2[m1[i1]] == (int32_t)i1) { vnMatches12[i1] = m1[i1]; ++nFound; }
        return nFound;
    }

    // ---- resident frames and the projection searches as whole functions ----------------------------------------------------
    // A Frame / KeyFrame kept in HBM between searches (orbm_frame): Frame::AssignFeaturesToGrid runs once, on the device.
    // Holds no reference to the arrays it was made from.  Movable, not copyable; any number of searches may read it at once.
    // mK and mDistCoef of a launch file (k3 = 0 when it has four coefficients).  k1 == 0: no undistortion (Frame.cc:421-425).
    struct Distortion {
        float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, k1 = 0.f, k2 = 0.f, p1 = 0.f, p2 = 0.f, k3 = 0.f;
        orbm_distortion c() const { return orbm_distortion{fx, fy, cx, cy, k1, k2, p1, p2, k3}; }
    };
    // Frame::ComputeImageBounds (Frame.cc:451-479), on the host; returns the status
    static int ImageBounds(const Distortion &cam, int width, int height, float &mnMinX, float &mnMinY, float &mnMaxX, float &mnMaxY)
    {
        const orbm_distortion c = cam.c();
        float b[4];
        const int rc = orbm_image_bounds(&c, width, height, b);
        if (rc == ORBX_OK) { mnMinX = b[0]; mnMinY = b[1]; mnMaxX = b[2]; mnMaxY = b[3]; }
        return rc;
    }

    class ResidentFrame {
    public:
        ResidentFrame() = default;
        explicit ResidentFrame(const FrameView &F) { mStatus = orbm_frame_create(F.mvKeysUn, F.mDescriptors, F.N, F.mvuRight, F.mnMinX, F.mnMinY, F.mnMaxX, F.mnMaxY, &mH); sync(); }
        // straight from the extractor's device results (no trip over PCIe): xyUndistorted = mvKeysUn coordinates (x0, y0, ...) or
        // null when the camera has no distortion; uRight from the host or from the last ComputeStereoMatches on `ex`
        ResidentFrame(ORBextractor &ex, const float *xyUndistorted, const float *uRight, bool uRightFromStereo, float mnMinX, float mnMinY,
                      float mnMaxX, float mnMaxY)
        {
            mStatus = orbm_frame_from_extractor(ex.handle(), 0, xyUndistorted, uRight, uRightFromStereo, mnMinX, mnMinY, mnMaxX, mnMaxY, &mH);
            sync();
        }
        // ... with Frame::UndistortKeyPoints done inside the frame build: the keypoints never leave the device
        ResidentFrame(ORBextractor &ex, const Distortion &cam, const float *uRight, bool uRightFromStereo, float mnMinX, float mnMinY,
                      float mnMaxX, float mnMaxY)
        {
            const orbm_distortion c = cam.c();
            mStatus = orbm_frame_from_extractor_cam(ex.handle(), 0, &c, uRight, uRightFromStereo, mnMinX, mnMinY, mnMaxX, mnMaxY, &mH);
            sync();
        }
        // frames first .. first + count - 1 of the extractor's last batch in ONE launch (orbm_frames_from_extractor); all or nothing:
        // an empty vector and *status (when given) say why.  cam null: the coordinates as the extractor left them.
        static std::vector<ResidentFrame> FromBatch(ORBextractor &ex, int first, int count, const Distortion *cam, bool uRightFromStereo,
                                                    float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, int *status = nullptr)
        {
            std::vector<orbm_frame *> h((size_t)(count > 0 ? count : 1), nullptr);
            orbm_distortion c = orbm_distortion();
            if (cam) c = cam->c();
            const int rc = orbm_frames_from_extractor(ex.handle(), first, count, cam ? &c : nullptr, uRightFromStereo, mnMinX, mnMinY, mnMaxX,
                                                      mnMaxY, h.data());
            if (status) *status = rc;
            std::vector<ResidentFrame> out;
            for (int i = 0; rc == ORBX_OK && i < count; ++i) {
                out.emplace_back();
                out.back().mH = h[i];
                out.back().sync();
            }
            return out;
        }
        // mvKeysUn coordinates by keypoint index (x0, y0, x1, ...): what the searches use
        std::vector<float> KeysUn() const
        {
            std::vector<float> xy((size_t)2 * (size_t)N);
            if (mH && orbm_frame_keypoints_un(mH, xy.data()) != ORBX_OK) xy.clear();
            return xy;
        }
        ResidentFrame(ResidentFrame &&o) noexcept : mH(o.mH), N(o.N), mStatus(o.mStatus) { o.mH = nullptr; }
        ResidentFrame &operator=(ResidentFrame &&o) noexcept { if (this != &o) { reset(); mH = o.mH; N = o.N; mStatus = o.mStatus; o.mH = nullptr; } return *this; }
        ResidentFrame(const ResidentFrame &) = delete;
        ResidentFrame &operator=(const ResidentFrame &) = delete;
        ~ResidentFrame() { reset(); }
        void reset() { if (mH) orbm_frame_destroy(mH); mH = nullptr; }
        const orbm_frame *handle() const { return mH; }
        int status() const { return mStatus; }
        int N = 0;
    private:
        void sync() { if (mStatus == ORBX_OK) orbm_frame_size(mH, &N, nullptr); else mH = nullptr; }
        orbm_frame *mH = nullptr;
        int mStatus = ORBX_OK;
    };
    // The flat form of a vector<MapPoint*> (orbm_points; see include/orbslam_hip.h for which form reads what): the binding fills it
    // in one pass over the pointer vector.
    struct PointList {
        std::vector<uint8_t> valid, desc, takes;
        std::vector<float> pos, normal, minDistance, maxDistance, angle;
        std::vector<int32_t> octave;
        void resize(size_t n, bool withRange, bool withNormal, bool withOctave)
        {
            valid.assign(n, 0); desc.resize(32 * n); takes.assign(n, 1); pos.resize(3 * n); angle.assign(n, 0.f);
            if (withRange) { minDistance.resize(n); maxDistance.resize(n); }
            if (withNormal) normal.resize(3 * n);
            if (withOctave) octave.assign(n, 0);
        }
        orbm_points view() const
        {
            orbm_points p;
            p.n = (int32_t)valid.size(); p.valid = valid.data(); p.pos = pos.data(); p.normal = normal.empty() ? nullptr : normal.data();
            p.min_distance = minDistance.empty() ? nullptr : minDistance.data(); p.max_distance = maxDistance.empty() ? nullptr : maxDistance.data();
            p.desc = desc.data(); p.takes = takes.empty() ? nullptr : takes.data(); p.octave = octave.empty() ? nullptr : octave.data();
            p.angle = angle.empty() ? nullptr : angle.data();
            return p;
        }
    };
    // Calibration + scale pyramid of the searched frame (Frame::fx .. mbf, mfLogScaleFactor, mvScaleFactors).
    struct Calibration {
        float fx = 0, fy = 0, cx = 0, cy = 0, mb = 0, mbf = 0, mfLogScaleFactor = 0;
        std::vector<float> mvScaleFactors;
        orbm_view view() const { return orbm_view{fx, fy, cx, cy, mb, mbf, mfLogScaleFactor, (int32_t)mvScaleFactors.size(), mvScaleFactors.data()}; }
    };
    // SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono) (ORBmatcher.cc:1529-1671),
    // whole.  Tcw / Tlw = mTcw of the two frames (4 x 4, row-major).  slotOwner[j] = entry of `last` whose point ends in
    // CurrentFrame.mvpMapPoints[j] (-1 untouched, -2 set to NULL by the rotation check); returns nmatches.
    int SearchByProjection(const ResidentFrame &Cur, const Calibration &K, const float *Tcw, const float *Tlw, const PointList &last,
                           const std::vector<uint8_t> &occupied, float th, bool bMono, std::vector<int32_t> &slotOwner)
    {
        const orbm_points p = last.view(); const orbm_view v = K.view();
        slotOwner.assign(Cur.N, -1); mScratch.resize(p.n);
        int nm = 0;
        mStatus = orbm_search_by_projection_last(Cur.handle(), &v, Tcw, Tlw, &p, occupied.empty() ? nullptr : occupied.data(), th, bMono, TH_HIGH,
                                                 mbCheckOrientation, slotOwner.data(), mScratch.data(), &nm, nullptr);
        return mStatus == ORBX_OK ? nm : 0;
    }
    // SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist) (:1673-1800), whole.
    int SearchByProjection(const ResidentFrame &Cur, const Calibration &K, const float *Tcw, const PointList &kf,
                           const std::vector<uint8_t> &occupied, float th, int ORBdist, std::vector<int32_t> &slotOwner)
    {
        const orbm_points p = kf.view(); const orbm_view v = K.view();
        slotOwner.assign(Cur.N, -1); mScratch.resize(p.n);
        int nm = 0;
        mStatus = orbm_search_by_projection_keyframe(Cur.handle(), &v, Tcw, &p, occupied.empty() ? nullptr : occupied.data(), th, ORBdist,
                                                     mbCheckOrientation, slotOwner.data(), mScratch.data(), &nm, nullptr);
        return mStatus == ORBX_OK ? nm : 0;
    }
    // SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
    // (:491-604), whole.  slotOwner[j] = list entry written to vpMatched[j] or -1.
    int SearchByProjection(const ResidentFrame &KF, const Calibration &K, const float *Scw, const PointList &points,
                           const std::vector<uint8_t> &occupied, int th, std::vector<int32_t> &slotOwner)
    {
        const orbm_points p = points.view(); const orbm_view v = K.view();
        slotOwner.assign(KF.N, -1); mScratch.resize(p.n);
        int nm = 0;
        mStatus = orbm_search_by_projection_sim3(KF.handle(), &v, Scw, &p, occupied.empty() ? nullptr : occupied.data(), th, TH_LOW,
                                                 slotOwner.data(), mScratch.data(), &nm, nullptr);
        return mStatus == ORBX_OK ? nm : 0;
    }
    // Tracking::SearchLocalPoints' data plane: isInFrustum for every listed point + SearchByProjection(Frame&, vector<MapPoint*>&, th)
    // (:46-132), whole.  projected[i] = what isInFrustum leaves in the MapPoint.
    int SearchLocalPoints(const ResidentFrame &Cur, const Calibration &K, const float *Tcw, const PointList &points,
                          const std::vector<uint8_t> &occupied, float th, std::vector<int32_t> &slotOwner,
                          std::vector<orbm_projected_point> *projected = nullptr)
    {
        const orbm_points p = points.view(); const orbm_view v = K.view();
        slotOwner.assign(Cur.N, -1); mScratch.resize(p.n);
        if (projected) projected->resize(p.n);
        int nm = 0;
        mStatus = orbm_search_by_projection_points(Cur.handle(), &v, Tcw, &p, occupied.empty() ? nullptr : occupied.data(), th, 0.5f, TH_HIGH,
                                                   mfNNratio, slotOwner.data(), mScratch.data(), &nm, projected ? projected->data() : nullptr, nullptr);
        return mStatus == ORBX_OK ? nm : 0;
    }
    // ---- a frame tracked in one call (mvInvLevelSigma2 = Frame::mvInvLevelSigma2: what the pose solve needs beside the Calibration)
    // Tracking::TrackWithMotionModel (src/Tracking.cc:1232-1284, behind UpdateLastFrame) in one call: SearchByProjection(Cur, Last,
    // th, bMono) with every slot free, again with 2 * th below minMatches, PoseOptimization from Tcw (the predicted pose, 4 x 4
    // row-major) over the matches, the counts of the discard loop.  slotOwner[j] as SearchByProjection(Cur, Last) leaves it (the
    // discard does not edit it); vbOutlier[j] is written only where slotOwner[j] >= 0; TcwOut[16] = what SetPose receives.
    orbm_track_result TrackWithMotionModel(const ResidentFrame &Cur, const Calibration &K, const std::vector<float> &mvInvLevelSigma2,
                                           const float *Tcw, const float *Tlw, const PointList &last, float th, bool bMono,
                                           std::vector<int32_t> &slotOwner, std::vector<uint8_t> &vbOutlier, float *TcwOut,
                                           int minMatches = 20)
    {
        const orbm_points p = last.view(); const orbm_view v = K.view();
        const orbm_pose_camera c = {K.fx, K.fy, K.cx, K.cy, K.mbf, (int32_t)mvInvLevelSigma2.size(), mvInvLevelSigma2.data()};
        slotOwner.assign(Cur.N, -1); vbOutlier.resize(Cur.N, 0); mScratch.resize(p.n);
        orbm_track_result r = {0, 0, 0, 0, 0, 0};
        mStatus = orbm_track_with_motion_model(Cur.handle(), &v, &c, Tcw, Tlw, &p, th, bMono, TH_HIGH, mbCheckOrientation, minMatches,
                                               slotOwner.data(), mScratch.data(), vbOutlier.data(), TcwOut, &r, nullptr);
        return r;
    }
    // Tracking::TrackLocalMap (src/Tracking.cc:1294-1320, behind UpdateLocalMap) in one call: SearchLocalPoints, PoseOptimization over
    // the union of the new matches and the slots the frame holds (baseHas / basePos / baseTakes by keypoint index: mvpMapPoints[j] !=
    // NULL, its GetWorldPos(), its Observations() > 0), the counts of the statistics loop (nmatches_map = mnMatchesInliers,
    // nmatches = the same with mbOnlyTracking).  vbOutlier[j] is written where the union holds a point.
    orbm_track_result TrackLocalMap(const ResidentFrame &Cur, const Calibration &K, const std::vector<float> &mvInvLevelSigma2, const float *Tcw,
                                    const PointList &points, const std::vector<uint8_t> &baseHas, const std::vector<float> &basePos,
                                    const std::vector<uint8_t> &baseTakes, float th, std::vector<int32_t> &slotOwner,
                                    std::vector<uint8_t> &vbOutlier, float *TcwOut, std::vector<orbm_projected_point> *projected = nullptr)
    {
        const orbm_points p = points.view(); const orbm_view v = K.view();
        const orbm_pose_camera c = {K.fx, K.fy, K.cx, K.cy, K.mbf, (int32_t)mvInvLevelSigma2.size(), mvInvLevelSigma2.data()};
        slotOwner.assign(Cur.N, -1); vbOutlier.resize(Cur.N, 0); mScratch.resize(p.n);
        if (projected) projected->resize(p.n);
        orbm_track_result r = {0, 0, 0, 0, 0, 0};
        const bool base = !baseHas.empty();
        mStatus = orbm_track_local_map(Cur.handle(), &v, &c, Tcw, &p, base ? baseHas.data() : nullptr, base ? basePos.data() : nullptr,
                                       base && !baseTakes.empty() ? baseTakes.data() : nullptr, th, 0.5f, TH_HIGH, mfNNratio, slotOwner.data(),
                                       mScratch.data(), projected ? projected->data() : nullptr, vbOutlier.data(), TcwOut, &r, nullptr);
        return r;
    }
    // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1303-1527), whole: vnMatches12[i1] = idx2 where both directions
    // agree (the entries of vpMatches12 the reference overwrites), else -1; returns nFound.
    int SearchBySim3(const ResidentFrame &KF1, const ResidentFrame &KF2, const Calibration &K, const float *T1w, const float *T2w, float s12,
                     const float *R12, const float *t12, const PointList &points1, const PointList &points2, float th,
                     std::vector<int32_t> &vnMatches12)
    {
        const orbm_points p1 = points1.view(), p2 = points2.view(); const orbm_view v = K.view();
        vnMatches12.assign(KF1.N, -1);
        int nf = 0;
        mStatus = orbm_search_by_sim3(KF1.handle(), KF2.handle(), &v, T1w, T2w, s12, R12, t12, &p1, &p2, th, TH_HIGH, nullptr, nullptr,
                                      vnMatches12.data(), &nf, nullptr, nullptr);
        return mStatus == ORBX_OK ? nf : 0;
    }

    // DBoW2::FeatureVector flattened in std::map order.
    struct FeatureVector {
        std::vector<int32_t> nodes, off, items;
        // from the per-feature node ids of orbm_bow_transform; keep[i] == 0: feature i is not in the vector
        static FeatureVector FromNodeIds(const std::vector<int32_t> &nodeId, const std::vector<uint8_t> *keep = nullptr)
        {
            std::vector<int32_t> idx;
            for (int32_t i = 0; i < (int32_t)nodeId.size(); ++i)
                if (!keep || (*keep)[i]) idx.push_back(i);
            std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return nodeId[a] < nodeId[b]; });
            FeatureVector fv;
            for (size_t k = 0; k < idx.size(); ++k) {
                if (k == 0 || nodeId[idx[k]] != nodeId[idx[k - 1]]) { fv.nodes.push_back(nodeId[idx[k]]); fv.off.push_back((int32_t)k); }
                fv.items.push_back(idx[k]);
            }
            fv.off.push_back((int32_t)idx.size());
            return fv;
        }
        // from the map ORBVocabulary::transform fills (Frame::mFeatVec / KeyFrame::mFeatVec)
        static FeatureVector FromMap(const DBoW2::FeatureVector &m)
        {
            FeatureVector fv;
            for (const auto &e : m) {
                fv.nodes.push_back((int32_t)e.first); fv.off.push_back((int32_t)fv.items.size());
                for (unsigned int i : e.second) fv.items.push_back((int32_t)i);
            }
            fv.off.push_back((int32_t)fv.items.size());
            return fv;
        }
    };

    // ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:360-489; valid2 == nullptr) and
    // SearchByBoW(KeyFrame*, KeyFrame*, ...) (:723-856).  valid = "owns a good MapPoint".
    int SearchByBoW(const FeatureVector &fv1, const std::vector<uint8_t> &valid1, const FrameView &KF1, const FeatureVector &fv2,
                    const std::vector<uint8_t> *valid2, const FrameView &F2, std::vector<int32_t> &vnMatches12)
    {
        std::vector<float> a1(KF1.N), a2(F2.N);
        for (int i = 0; i < KF1.N; ++i) a1[i] = KF1.mvKeysUn[i].angle;
        for (int i = 0; i < F2.N; ++i) a2[i] = F2.mvKeysUn[i].angle;
        vnMatches12.assign(KF1.N, -1);
        int nm = 0;
        mStatus = orbm_search_by_bow(fv1.nodes.data(), fv1.off.data(), fv1.items.data(), (int)fv1.nodes.size(), valid1.data(),
                                     KF1.mDescriptors, a1.data(), KF1.N, fv2.nodes.data(), fv2.off.data(), fv2.items.data(),
                                     (int)fv2.nodes.size(), valid2 ? valid2->data() : nullptr, F2.mDescriptors, a2.data(), F2.N,
                                     TH_LOW, valid2 ? 1 : 0, mfNNratio, mbCheckOrientation, vnMatches12.data(), nullptr, &nm);
        return mStatus == ORBX_OK ? nm : 0;
    }

    // The same on two resident frames: nothing but the feature-vector lists travels with the call.
    int SearchByBoW(const FeatureVector &fv1, const std::vector<uint8_t> &valid1, const ResidentFrame &KF1, const FeatureVector &fv2,
                    const std::vector<uint8_t> *valid2, const ResidentFrame &F2, std::vector<int32_t> &vnMatches12)
    {
        vnMatches12.assign(KF1.N, -1);
        int nm = 0;
        mStatus = orbm_frame_search_by_bow(KF1.handle(), fv1.nodes.data(), fv1.off.data(), fv1.items.data(), (int)fv1.nodes.size(),
                                           valid1.data(), F2.handle(), fv2.nodes.data(), fv2.off.data(), fv2.items.data(),
                                           (int)fv2.nodes.size(), valid2 ? valid2->data() : nullptr, TH_LOW, valid2 ? 1 : 0, mfNNratio,
                                           mbCheckOrientation, vnMatches12.data(), nullptr, &nm);
        return mStatus == ORBX_OK ? nm : 0;
    }

    // One side of a batched SearchByBoW: a resident frame, its flat FeatureVector and its "owns a good MapPoint" mask
    // (valid == nullptr on the second side: SearchByBoW(KeyFrame*, Frame&, ...), every feature of the frame is a candidate).
    struct BoWSide {
        const ResidentFrame *frame; const FeatureVector *fv; const std::vector<uint8_t> *valid;
    };
    // SearchByBoW for K (first, second) pairs in ONE call (orbm_frame_search_by_bow_pairs; at most 64): the loop over the candidate
    // keyframes of Tracking::Relocalization (Tracking.cc:1768-1795: second = the current frame in every pair, bKeyFrames = false)
    // and of LoopClosing::ComputeSim3 (LoopClosing.cc:252-280: first = the current keyframe in every pair, bKeyFrames = true: both
    // masks, bestDist1 < TH_LOW).  vvnMatches12[k] / vnMatches[k] = what the single call returns for pair k.  Returns the status.
    int SearchByBoW(const std::vector<std::pair<BoWSide, BoWSide>> &vPairs, bool bKeyFrames, std::vector<std::vector<int32_t>> &vvnMatches12,
                    std::vector<int32_t> &vnMatches)
    {
        const size_t K = vPairs.size();
        std::vector<orbm_bow_pair> p(K);
        vvnMatches12.resize(K);
        vnMatches.assign(K > 0 ? K : 1, 0);
        for (size_t k = 0; k < K; ++k) {
            const BoWSide &a = vPairs[k].first, &b = vPairs[k].second;
            vvnMatches12[k].assign(a.frame->N > 0 ? a.frame->N : 1, -1);
            p[k].frame1 = a.frame->handle(); p[k].nodes1 = a.fv->nodes.data(); p[k].off1 = a.fv->off.data(); p[k].items1 = a.fv->items.data();
            p[k].nn1 = (int32_t)a.fv->nodes.size(); p[k].valid1 = a.valid->data();
            p[k].frame2 = b.frame->handle(); p[k].nodes2 = b.fv->nodes.data(); p[k].off2 = b.fv->off.data(); p[k].items2 = b.fv->items.data();
            p[k].nn2 = (int32_t)b.fv->nodes.size(); p[k].valid2 = bKeyFrames && b.valid ? b.valid->data() : nullptr;
            p[k].match12 = vvnMatches12[k].data(); p[k].match21 = nullptr;
        }
        mStatus = orbm_frame_search_by_bow_pairs(p.data(), (int)K, TH_LOW, bKeyFrames ? 1 : 0, mfNNratio, mbCheckOrientation, vnMatches.data());
        for (size_t k = 0; k < K; ++k) vvnMatches12[k].resize(vPairs[k].first.frame->N);
        vnMatches.resize(K);
        return mStatus;
    }

    // SearchForTriangulation on two resident keyframes (stereo = the frame's right coordinate >= 0): the lists and the two
    // "owns a MapPoint" masks are all that travels.
    int SearchForTriangulation(const ResidentFrame &KF1, const FeatureVector &fv1, const std::vector<uint8_t> &hasMP1,
                               const ResidentFrame &KF2, const FeatureVector &fv2, const std::vector<uint8_t> &hasMP2, const float F12[9],
                               float ex, float ey, bool bOnlyStereo, const std::vector<float> &scaleFactors2,
                               const std::vector<float> &levelSigma2, std::vector<std::pair<size_t, size_t>> &vMatchedPairs)
    {
        vMatchedPairs.clear();
        std::vector<int32_t> m12(KF1.N > 0 ? KF1.N : 1, -1);
        int nm = 0;
        mStatus = orbm_frame_search_for_triangulation(KF1.handle(), fv1.nodes.data(), fv1.off.data(), fv1.items.data(), (int)fv1.nodes.size(),
                                                      hasMP1.data(), KF2.handle(), fv2.nodes.data(), fv2.off.data(), fv2.items.data(),
                                                      (int)fv2.nodes.size(), hasMP2.data(), bOnlyStereo ? 1 : 0, F12, ex, ey,
                                                      scaleFactors2.data(), levelSigma2.data(), (int)scaleFactors2.size(),
                                                      mbCheckOrientation, m12.data(), &nm);
        if (mStatus != ORBX_OK) return 0;
        for (int i = 0; i < KF1.N; ++i)
            if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);
        return (int)vMatchedPairs.size();
    }

    // LocalMapping::CreateNewMapPoints' loop over the neighbour keyframes (LocalMapping.cc:281-517) in one call
    // (orbm_create_new_map_points): the searches, triangulations and gates of all neighbours in one launch.  The neighbours are
    // the ones that passed the baseline test, in the reference's order.  Returns the creation list in the reference's order
    // ((k, idx1) ascending) and the reject counters; one call cannot be interrupted between neighbours -- a caller that needs
    // CheckNewKeyFrames() in between calls with the neighbours in chunks.
    struct TriangKeyFrame {
        const ResidentFrame *frame;
        const float *Tcw;                          // 4 x 4 row-major
        float fx, fy, cx, cy, invfx, invfy, mb, mbf;
        const float *depth;                        // mvDepth, or nullptr if no keypoint of the frame is stereo
        const std::vector<uint8_t> *hasMP;
        const FeatureVector *fv;
    };
    struct Neighbour { TriangKeyFrame kf; float F12[9]; float ex, ey; };
    struct NewPoint { int k; int idx1, idx2; float x3D[3]; };
    struct NewPointCounters { int nnew = 0, nTriangulationRejects = 0, nParalaxRejects = 0, nDepthRejects = 0, nRepErrorRejects = 0, nScaleConsRejects = 0; };
    int CreateNewMapPoints(const TriangKeyFrame &cur, const std::vector<float> &scaleFactors, const std::vector<float> &levelSigma2,
                           float scaleFactor, const std::vector<Neighbour> &neighbours, std::vector<NewPoint> &created,
                           NewPointCounters &counters)
    {
        created.clear();
        counters = NewPointCounters();
        const int K = (int)neighbours.size(), n1 = cur.frame->N;
        auto flat = [](const TriangKeyFrame &k, const float *F12, float ex, float ey) {
            orbm_triang_keyframe o;
            o.frame = k.frame->handle(); o.Tcw = k.Tcw;
            o.fx = k.fx; o.fy = k.fy; o.cx = k.cx; o.cy = k.cy; o.invfx = k.invfx; o.invfy = k.invfy; o.mb = k.mb; o.mbf = k.mbf;
            o.depth = k.depth; o.has_mappoint = k.hasMP->data();
            o.nodes = k.fv->nodes.data(); o.off = k.fv->off.data(); o.items = k.fv->items.data(); o.nn = (int32_t)k.fv->nodes.size();
            o.F12 = F12; o.ex = ex; o.ey = ey;
            return o;
        };
        const orbm_triang_keyframe c = flat(cur, nullptr, 0.f, 0.f);
        std::vector<orbm_triang_keyframe> nb;
        for (const Neighbour &n : neighbours) nb.push_back(flat(n.kf, n.F12, n.ex, n.ey));
        const size_t kn = (size_t)K * (size_t)(n1 > 0 ? n1 : 0);
        std::vector<int32_t> m12(kn ? kn : 1, -1), counts((size_t)(K ? K : 1) * ORBM_TRI_NSTATUS, 0);
        std::vector<int8_t> status(kn ? kn : 1, (int8_t)ORBM_TRI_NO_MATCH);
        std::vector<float> x3d(3 * (kn ? kn : 1), 0.f);
        int nnew = 0;
        mStatus = orbm_create_new_map_points(&c, nb.data(), K, scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(), scaleFactor,
                                             m12.data(), status.data(), x3d.data(), counts.data(), &nnew);
        if (mStatus != ORBX_OK) return 0;
        for (size_t o = 0; o < kn; ++o)
            if (status[o] == ORBM_TRI_CREATED)
                created.push_back({(int)(o / (size_t)n1), (int)(o % (size_t)n1), m12[o], {x3d[3 * o], x3d[3 * o + 1], x3d[3 * o + 2]}});
        for (int k = 0; k < K; ++k) {
            const int32_t *ck = counts.data() + (size_t)k * ORBM_TRI_NSTATUS;
            counters.nTriangulationRejects += ck[ORBM_TRI_SVD_ZERO]; counters.nParalaxRejects += ck[ORBM_TRI_PARALLAX];
            counters.nDepthRejects += ck[ORBM_TRI_DEPTH]; counters.nRepErrorRejects += ck[ORBM_TRI_REPROJ1];
            counters.nScaleConsRejects += ck[ORBM_TRI_SCALE];
        }
        counters.nnew = nnew;
        return nnew;
    }

    // ORBmatcher::SearchForTriangulation (ORBmatcher.cc:858-1024).  The FeatureVector co-iteration builds the candidate
    // list of every keypoint of KF1 (the members of the same vocabulary node in KF2, in member order), the device
    // runs the loop with its epipolar gates, the rotation histogram and the pair list are finished here.
    // hasMP / stereo: "pKF->GetMapPoint(idx) exists" and "mvuRight[idx] >= 0", one byte per keypoint.
    int SearchForTriangulation(const FrameView &KF1, const FeatureVector &fv1, const std::vector<uint8_t> &hasMP1,
                               const std::vector<uint8_t> &stereo1, const FrameView &KF2, const FeatureVector &fv2,
                               const std::vector<uint8_t> &hasMP2, const std::vector<uint8_t> &stereo2, const float F12[9],
                               float ex, float ey, bool bOnlyStereo, const std::vector<float> &scaleFactors2,
                               const std::vector<float> &levelSigma2, std::vector<std::pair<size_t, size_t>> &vMatchedPairs)
    {
        vMatchedPairs.clear();
        std::vector<int32_t> node_of(KF1.N, -1);       // position in fv2.nodes of keypoint i's node, if both frames have it
        for (size_t a = 0, b = 0; a < fv1.nodes.size() && b < fv2.nodes.size();) {
            if (fv1.nodes[a] == fv2.nodes[b]) {
                for (int32_t k = fv1.off[a]; k < fv1.off[a + 1]; ++k) node_of[fv1.items[k]] = (int32_t)b;
                ++a; ++b;
            } else if (fv1.nodes[a] < fv2.nodes[b]) ++a;
            else ++b;
        }
        std::vector<int32_t> off(KF1.N + 1, 0), idx;
        for (int i = 0; i < KF1.N; ++i) {
            if (node_of[i] >= 0) idx.insert(idx.end(), fv2.items.begin() + fv2.off[node_of[i]], fv2.items.begin() + fv2.off[node_of[i] + 1]);
            off[i + 1] = (int32_t)idx.size();
        }
        std::vector<int32_t> m12(KF1.N, -1), bd(KF1.N, 0);
        mStatus = orbm_match_triangulation(KF1.mvKeysUn, KF1.mDescriptors, KF1.N, KF2.mvKeysUn, KF2.mDescriptors, KF2.N, off.data(),
                                           idx.data(), hasMP1.data(), hasMP2.data(), stereo1.data(), stereo2.data(), bOnlyStereo ? 1 : 0,
                                           F12, ex, ey, scaleFactors2.data(), levelSigma2.data(), (int)scaleFactors2.size(), m12.data(),
                                           bd.data());
        if (mStatus != ORBX_OK) return 0;
        int nmatches = 0;
        for (int i = 0; i < KF1.N; ++i) nmatches += m12[i] >= 0;
        if (mbCheckOrientation) {                      // :965-976, :992-1011
            std::vector<std::vector<int>> rotHist(HISTO_LENGTH);
            const float factor = 1.0f / HISTO_LENGTH;
            for (int i = 0; i < KF1.N; ++i) {
                if (m12[i] < 0) continue;
                float rot = KF1.mvKeysUn[i].angle - KF2.mvKeysUn[m12[i]].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round(rot * factor);
                if (bin == HISTO_LENGTH) bin = 0;
                rotHist[bin].push_back(i);
            }
            int ind1, ind2, ind3;
            ComputeThreeMaxima(rotHist, ind1, ind2, ind3);
            for (int b = 0; b < HISTO_LENGTH; ++b) {
                if (b == ind1 || b == ind2 || b == ind3) continue;
                for (int i : rotHist[b]) { m12[i] = -1; --nmatches; }
            }
        }
        for (int i = 0; i < KF1.N; ++i)
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return nmatches;
    }

    // ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1802-1843) on the bin sizes.
    static void ComputeThreeMaxima(const std::vector<std::vector<int>> &histo, int &ind1, int &ind2, int &ind3)
    {
        int max1 = 0, max2 = 0, max3 = 0;
        ind1 = ind2 = ind3 = -1;
        for (int i = 0; i < (int)histo.size(); ++i) {
            const int s = (int)histo[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) ind3 = -1;
    }

    // The fork's SearchByProjection(Frame&, Map*, Rcw, tcw, ...) over every map point (ORBmatcher.cc:134-222): isInFrustum,
    // level prediction, windowed search and acceptance on the device.  mp*: one entry per map point (position and normal
    // xyz, distance invariance limits, MapPoint::GetDescriptor()); vMatchedMPs[j] = map point index for keypoint j or -1.
    int SearchByProjection(const FrameView &F, const std::vector<uint8_t> &hasMapPoint, const float *mpPos, const float *mpNormal,
                           const float *mpMinDistance, const float *mpMaxDistance, const uint8_t *mpDescriptors, int nMapPoints,
                           const double Rcw[9], const double tcw[3], const orbm_camera &cam, const std::vector<float> &scaleFactors,
                           float th, std::vector<int32_t> &vMatchedMPs)
    {
        vMatchedMPs.assign(F.N, -1);
        int nm = 0;
        mStatus = orbm_search_by_projection_map(F.mvKeysUn, F.mDescriptors, F.N, hasMapPoint.data(), mpPos, mpNormal, mpMinDistance,
                                                mpMaxDistance, mpDescriptors, nMapPoints, Rcw, tcw, &cam, scaleFactors.data(),
                                                (int)scaleFactors.size(), th, mfNNratio, TH_RELOC, vMatchedMPs.data(), &nm, nullptr);
        return mStatus == ORBX_OK ? nm : 0;
    }

    // What pMap->GetAllMapPoints() returned, flat and resident in HBM (orbm_map): made once per Tracking::Relocalization(), read by
    // the searches of every candidate keyframe's PnPsolver::iterate.  Immutable; holds no reference to the arrays it was made from.
    // Movable, not copyable; any number of searches may read it at once.
    class MapSnapshot {
    public:
        MapSnapshot() = default;
        MapSnapshot(const float *mpPos, const float *mpNormal, const float *mpMinDistance, const float *mpMaxDistance,
                    const uint8_t *mpDescriptors, int nMapPoints)
        {
            mStatus = orbm_map_create(mpPos, mpNormal, mpMinDistance, mpMaxDistance, mpDescriptors, nMapPoints, &mH);
            if (mStatus == ORBX_OK) orbm_map_size(mH, &N); else mH = nullptr;
        }
        MapSnapshot(MapSnapshot &&o) noexcept : N(o.N), mH(o.mH), mStatus(o.mStatus) { o.mH = nullptr; }
        MapSnapshot &operator=(MapSnapshot &&o) noexcept { if (this != &o) { reset(); mH = o.mH; N = o.N; mStatus = o.mStatus; o.mH = nullptr; } return *this; }
        MapSnapshot(const MapSnapshot &) = delete;
        MapSnapshot &operator=(const MapSnapshot &) = delete;
        ~MapSnapshot() { reset(); }
        void reset() { if (mH) orbm_map_destroy(mH); mH = nullptr; }
        const orbm_map *handle() const { return mH; }
        int status() const { return mStatus; }
        int N = 0;
    private:
        orbm_map *mH = nullptr;
        int mStatus = ORBX_OK;
    };
    struct MapPose { double Rcw[9], tcw[3]; };      // row-major Rcw

    // The search above under every pose of `poses` (at most 16) in ONE launch (orbm_frame_search_by_projection_map_poses):
    // vMatchedMPs[p] and nmatches[p] are what the single-pose search returns for poses[p].  False (and empty rows) on failure.
    bool SearchByProjection(const ResidentFrame &F, const std::vector<uint8_t> &hasMapPoint, const MapSnapshot &map,
                            const std::vector<MapPose> &poses, const orbm_camera &cam, const std::vector<float> &scaleFactors, float th,
                            std::vector<std::vector<int32_t>> &vMatchedMPs, std::vector<int> &nmatches)
    {
        const int P = (int)poses.size(), n = F.N;
        std::vector<double> R((size_t)9 * P + 1), t((size_t)3 * P + 1);
        for (int p = 0; p < P; ++p) {
            std::copy(poses[p].Rcw, poses[p].Rcw + 9, R.begin() + 9 * p);
            std::copy(poses[p].tcw, poses[p].tcw + 3, t.begin() + 3 * p);
        }
        std::vector<int32_t> rows((size_t)P * n + 1, -1), nm((size_t)P + 1, 0);
        mStatus = orbm_frame_search_by_projection_map_poses(F.handle(), hasMapPoint.empty() ? nullptr : hasMapPoint.data(), map.handle(), R.data(),
                                                            t.data(), P, &cam, scaleFactors.data(), (int)scaleFactors.size(), th, mfNNratio,
                                                            TH_RELOC, rows.data(), nm.data(), nullptr);
        vMatchedMPs.clear(); nmatches.clear();
        if (mStatus != ORBX_OK) return false;
        for (int p = 0; p < P; ++p) {
            vMatchedMPs.emplace_back(rows.begin() + (size_t)p * n, rows.begin() + (size_t)(p + 1) * n);
            nmatches.push_back(nm[p]);
        }
        return true;
    }
    // ... on a frame given as host arrays: its grid is built for this call (a Frame that is searched again keeps a ResidentFrame)
    bool SearchByProjection(const FrameView &F, const std::vector<uint8_t> &hasMapPoint, const MapSnapshot &map,
                            const std::vector<MapPose> &poses, const orbm_camera &cam, const std::vector<float> &scaleFactors, float th,
                            std::vector<std::vector<int32_t>> &vMatchedMPs, std::vector<int> &nmatches)
    {
        const ResidentFrame R(F);
        if (R.status() != ORBX_OK) { mStatus = R.status(); vMatchedMPs.clear(); nmatches.clear(); return false; }
        return SearchByProjection(R, hasMapPoint, map, poses, cam, scaleFactors, th, vMatchedMPs, nmatches);
    }

    // MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:305-370) for many map points at once: the observed descriptors of
    // point i are rows off[i] .. off[i+1) of desc; best[i] = the row (within the point) with the least median distance.
    static int ComputeDistinctiveDescriptors(const uint8_t *desc, const std::vector<int32_t> &off, std::vector<int32_t> &best)
    {
        best.assign(off.empty() ? 0 : off.size() - 1, -1);
        return best.empty() ? ORBX_OK : orbm_distinctive_descriptors(desc, off.data(), (int)best.size(), best.data());
    }

    int status() const { return mStatus; }

protected:
    float mfNNratio;
    bool mbCheckOrientation;
    int mStatus = ORBX_OK;
    int mFuseKeyFramesWaits = 0, mFuseKeyFramesRefreshes = 0;      // of the last FuseKeyFrames / FuseKeyFramesSim3
    std::vector<int32_t> mScratch;     // per-entry output of the whole-function searches (not re-entrant per OBJECT; instances are stack-local, as in the reference)
};

// ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h:31) as the
// front end uses it: loadFromTextFile (System.cc:69) and transform (Frame.cc:410-417).  The tree lives in HBM
// behind orbm_vocab_create; the descent of all features of a frame is one device call, the two std::map
// results are filled here in feature order like TemplatedVocabulary.h:1127-1160.
class ORBVocabulary {
    typedef DBoW2::BowVector BowVector;
    typedef DBoW2::FeatureVector FeatureVector;


public:
    ORBVocabulary() {}
    ~ORBVocabulary() { clear(); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;

    // Text layout of TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1420): header `k L scoring
    // weighting`, then per node `parent isLeaf d0..d31 weight`; node ids are line numbers, word ids count the leaves.
    bool loadFromTextFile(const std::string &filename) {
        clear();
        FILE *f = std::fopen(filename.c_str(), "r");
        if (!f) return false;
        int k = 0, L = 0, n1 = 0, n2 = 0;
        bool ok = std::fscanf(f, "%d %d %d %d", &k, &L, &n1, &n2) == 4 && !(k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3);
        std::vector<int32_t> parent(1, 0), word(1, -1);
        std::vector<uint8_t> desc(32, 0);
        std::vector<double> weight(1, 0.0);
        int nwords = 0;
        while (ok) {
            int pid, leaf;
            if (std::fscanf(f, "%d %d", &pid, &leaf) != 2) break;            // end of file
            const int id = (int)parent.size();
            if (pid < 0 || pid >= id) { ok = false; break; }
            unsigned b[32];
            for (int i = 0; i < 32 && ok; ++i) ok = std::fscanf(f, "%u", &b[i]) == 1 && b[i] < 256;
            double w = 0;
            ok = ok && std::fscanf(f, "%lf", &w) == 1;
            if (!ok) break;
            parent.push_back(pid); word.push_back(leaf > 0 ? nwords++ : -1); weight.push_back(w);
            for (int i = 0; i < 32; ++i) desc.push_back((uint8_t)b[i]);
        }
        std::fclose(f);
        if (!ok) return false;
        const int n = (int)parent.size();
        std::vector<int32_t> off(n + 1, 0), ids(n - 1), fill(n, 0);
        for (int i = 1; i < n; ++i) ++off[parent[i] + 1];
        for (int i = 0; i < n; ++i) off[i + 1] += off[i];
        for (int i = 1; i < n; ++i) ids[off[parent[i]] + fill[parent[i]]++] = i;   // children in order of appearance
        m_k = k; m_L = L; m_scoring = n1; m_weighting = n2; m_nwords = nwords; m_nnodes = n;
        mStatus = orbm_vocab_create(off.data(), ids.data(), desc.data(), word.data(), weight.data(), n, L, &mVoc);
        return mStatus == ORBX_OK;
    }

    bool empty() const { return m_nwords == 0; }
    unsigned int size() const { return (unsigned int)m_nwords; }
    int getBranchingFactor() const { return m_k; }
    int getDepthLevels() const { return m_L; }

    // features: n x 32 bytes (Converter::toDescriptorVector of mDescriptors is this, row by row).
    void transform(const uint8_t *features, int n, BowVector &v, FeatureVector &fv, int levelsup) {
        v.clear(); fv.clear();
        if (!mVoc || n <= 0) return;
        mWord.resize(n); mNode.resize(n); mW.resize(n);
        mStatus = orbm_bow_transform(mVoc, features, n, levelsup, mWord.data(), mNode.data(), mW.data());
        if (mStatus != ORBX_OK) return;
        const bool tf = m_weighting == 0 || m_weighting == 1;                // TF_IDF / TF accumulate, IDF / BINARY keep the first
        for (int i = 0; i < n; ++i)
            if (mW[i] > 0) {                                                 // not stopped
                if (tf) v[(unsigned)mWord[i]] += mW[i];                      // BowVector::addWeight
                else v.insert(BowVector::value_type((unsigned)mWord[i], mW[i]));   // BowVector::addIfNotExist
                fv[(unsigned)mNode[i]].push_back((unsigned)i);               // FeatureVector::addFeature
            }
        const bool must = m_scoring != 5;                                    // every scoring but DOT_PRODUCT normalises (ScoringObject.h:74-89)
        if (tf && !v.empty() && !must) {
            const double nd = (double)v.size();
            for (auto &e : v) e.second /= nd;
        }
        if (must) {                                                          // BowVector::normalize: L2 for L2_NORM, else L1
            double norm = 0;
            if (m_scoring == 1) { for (auto &e : v) norm += e.second * e.second; norm = std::sqrt(norm); }
            else for (auto &e : v) norm += std::fabs(e.second);
            if (norm > 0) for (auto &e : v) e.second /= norm;
        }
    }

    orbm_vocabulary *handle() const { return mVoc; }
    int status() const { return mStatus; }

private:
    void clear() { if (mVoc) orbm_vocab_destroy(mVoc); mVoc = nullptr; m_nwords = m_nnodes = 0; }
    orbm_vocabulary *mVoc = nullptr;
    int m_k = 0, m_L = 0, m_scoring = 0, m_weighting = 0, m_nwords = 0, m_nnodes = 0, mStatus = ORBX_OK;
    std::vector<int32_t> mWord, mNode;
    std::vector<double> mW;
};

// Numeric core of FEA2: the members and methods g2o and Optimizer touch
// (FEA2.h: K-size, vva, vvf, sE, nsE; Set/Compute* calls at
// optimization_algorithm_levenberg.cpp:159-199).
class FEA2 {
public:
    FEA2(unsigned int input_E, float input_nu, float input_h, float input_fg1, int input_nElType)
        : E(input_E), nu(input_nu), h(input_h), fg(input_fg1), nElType(input_nElType) {}
    ~FEA2() { fem_destroy(mModel); }
    FEA2(const FEA2 &) = delete;
    FEA2 &operator=(const FEA2 &) = delete;

    // SetSecondLayer + Set_u0 + MatrixAssemblyC3D8/6 + ImposeDirichletEncastre_K
    // (the numeric half of FEA2::Compute(1), FEA2.cc:92-103) for a top-layer mesh:
    // faces = triangles (nElType 2) or quads (nElType 1).
    bool Compute(const std::vector<float> &topXYZ, const std::vector<int32_t> &faces)
    {
        const int nTop = (int)topXYZ.size() / 3, nv = nElType == 1 ? 4 : 3, nf = (int)faces.size() / nv;
        std::vector<float> nodes((size_t)6 * nTop);
        fem_second_layer(topXYZ.data(), nTop, h, nodes.data());
        u0 = nodes;
        std::vector<int32_t> elems((size_t)nf * 2 * nv);
        for (int f = 0; f < nf; ++f)
            for (int k = 0; k < nv; ++k) {
                elems[(size_t)f * 2 * nv + k] = faces[(size_t)f * nv + k];
                elems[(size_t)f * 2 * nv + nv + k] = faces[(size_t)f * nv + k] + nTop; // FEA2.cc:1392-1399
            }
        fem_destroy(mModel);
        mModel = nullptr;
        mTrialReady = false;
        mStatus = fem_create(nElType == 1 ? FEM_C3D8 : FEM_C3D6, nodes.data(), 1, 2 * nTop, elems.data(), nf, E, nu, fg, &mModel);
        if (mStatus != ORBX_OK) return false; // Ksize<=3: assembly refuses (:1386)
        Ksize = 6 * nTop;
        vDir.resize(nTop);
        for (int i = 0; i < nTop; ++i) vDir[i] = nTop + i; // vvDir_t, :1198
        if ((mStatus = fem_assemble(mModel)) != ORBX_OK) return false;
        mStatus = fem_dirichlet_penalty(mModel, vDir.data(), nTop, 100000000.0f);
        return mStatus == ORBX_OK;
    }

    // Set_uf (top layer moved, bottom layer kept) + ComputeDisplacement (:1732-1808)
    void ComputeDisplacement(const std::vector<float> &topXYZ_new)
    {
        std::vector<float> uf = u0;
        std::memcpy(uf.data(), topXYZ_new.data(), sizeof(float) * topXYZ_new.size());
        vva.resize(Ksize);
        mStatus = fem_displacement(mModel, uf.data(), u0.data(), vDir.data(), (int)vDir.size(), 100000000.0f, vva.data());
    }
    void ComputeForces() { vvf.resize(Ksize); mStatus = fem_matvec(mModel, vva.data(), vvf.data()); }
    float ComputeStrainEnergy() { mStatus = fem_strain_energy(mModel, vva.data(), &sE, &nsE); return sE; }
    float NormalizeStrainEnergy() const { return nsE; }

    // The whole per-trial sequence of the LM hook (optimization_algorithm_levenberg.cpp:159-175)
    // in one call, K / u0 / Dirichlet list resident: vertex estimates in, nsE out.
    float TrialEnergy(const std::vector<double> &vertexXYZ)
    {
        if (!mTrialReady) {
            mStatus = fem_trial_setup(mModel, u0.data(), vDir.data(), (int)vDir.size(), 100000000.0f, (int)vertexXYZ.size() / 3, nullptr, 0);
            mTrialReady = mStatus == ORBX_OK;
        }
        if (mTrialReady) mStatus = fem_trial_energy(mModel, vertexXYZ.data(), nullptr, &sE, &nsE);
        return nsE;
    }

    unsigned int E;
    float nu, h, fg;
    int nElType, Ksize = 0;
    float sE = 0.f, nsE = 0.f;
    std::vector<float> u0, vva, vvf;
    std::vector<int32_t> vDir;
    int status() const { return mStatus; }
    fem_model *model() { return mModel; }

private:
    fem_model *mModel = nullptr;
    int mStatus = ORBX_OK;
    bool mTrialReady = false;
};

// The FEM side of Optimizer::PoseOptimizationNR (src/Optimizer.cc:478-834) as one compiled sequence:
//   FEA2 fea2(mnId, 3500, 0.495, 0.5, 0.577350269, nElType)                       :480
//   fea2.Compute(1)                                                               :723   -> Compute()
//   4 x { optimizer.initializeOptimization(0); optimizer.optimize(10); classify } :733-790 -> Optimize()
// and, inside every Levenberg iteration of optimize(), g2o's trial loop with this fork's hook
// (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:63-232; the hook :159-199) -> Iteration() / Hook().
// What g2o computes -- the reprojection chi2, the linear solve, the vertex estimates, push / pop -- stays g2o's and
// comes in through `Problem` (a g2o::SparseOptimizer + BlockSolver in the real build, a scripted stand-in in the tests):
//   void   initializeOptimization(int round)          optimizer.initializeOptimization(0)              Optimizer.cc:738
//   double activeRobustChi2()                         computeActiveErrors() + activeRobustChi2()       levenberg.cpp:80-99
//   void   buildSystem()                              _solver->buildSystem()                           :102
//   double computeLambdaInit()                        :242-256
//   void   push(), pop(), discardTop()                _optimizer->push() / pop() / discardTop()        :123, 222, 216
//   bool   solveAndUpdate(double lambda)              setLambda, solve, update(x), restoreDiagonal     :130-146 (-> ok2)
//   double computeScale(double lambda)                :258-267
//   void   pointEstimates(std::vector<double> &xyz)   GetPointCoordinates(pFEA2->vVertices)            :293-311
//   bool   terminate()                                _optimizer->terminate()
//   void   classifyOutliers(int round)                the inlier / outlier pass after each round       Optimizer.cc:752-790
class PoseOptimizationNR_fem {
public:
    struct Trial { float sE, nsE; double tempChi, currentChi, rho, lambda; int qmax, accepted; };
    enum SolverResult { Terminate = 2, OK = 1, Fail = -1 };   // OptimizationAlgorithm::SolverResult

    explicit PoseOptimizationNR_fem(int nElType) : fea2(3500, 0.495f, 0.5f, 0.577350269f, nElType) {}

    // fea2.Compute(1), Optimizer.cc:723 (its numeric half: the PCL meshing in front stays the reference's), and the
    // state of the hook parked on the device: u0, the Dirichlet list, the optimiser's nVertices point vertices and
    // vNewPointsBase (derived[nDerived][4] = {2 | 3, i0, i1, i2}; nVertices + nDerived = top-layer nodes).
    bool Compute(const std::vector<float> &topXYZ, const std::vector<int32_t> &faces, int nVertices,
                 const std::vector<int32_t> &derived = std::vector<int32_t>())
    {
        if (!fea2.Compute(topXYZ, faces)) return false;
        mStatus = fem_trial_setup(fea2.model(), fea2.u0.data(), fea2.vDir.data(), (int)fea2.vDir.size(), 100000000.0f, nVertices,
                                  derived.empty() ? nullptr : derived.data(), (int)derived.size() / 4);
        mNV = nVertices;
        return mStatus == ORBX_OK;
    }

    // The hook, levenberg.cpp:159-199: GetPointCoordinates + Set_uf + ComputeDisplacement + ComputeForces +
    // ComputeStrainEnergy + NormalizeStrainEnergy in one device call, then g2o's weighting, verbatim.
    double Hook(const std::vector<double> &vertexXYZ, int qmax, double tempChi, double &currentChi, float &sE, float &nsE)
    {
        sE = 0.0f; nsE = 0.0f;
        mStatus = fem_trial_energy(fea2.model(), vertexXYZ.data(), nullptr, &sE, &nsE);     // :164-171
        float w_rE = 1.0;                                                                    // :184
        float w_sE = 5.0;                                                                    // :185
        if (qmax == 0) {                                                                     // :186-193
            w_rE = 1.0;
            w_sE = 2.0;
            currentChi += nsE;
        }
        return w_rE * tempChi + w_sE * nsE;                                                  // :198
    }

    // One Levenberg iteration = OptimizationAlgorithmLevenberg::solve(iteration), levenberg.cpp:63-232, bInFEA set.
    template <class Problem>
    SolverResult Iteration(Problem &g2o, int iteration, std::vector<Trial> *log = nullptr)
    {
        double currentChi = g2o.activeRobustChi2();            // :80-97
        double tempChi = currentChi;
        const double iniChi = currentChi;
        g2o.buildSystem();                                     // :102
        if (iteration == 0) {                                  // :109-114
            mLambda = g2o.computeLambdaInit();
            mNi = 2;
            mNBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        std::vector<double> pts;
        do {
            g2o.push();                                        // :123
            const bool ok2 = g2o.solveAndUpdate(mLambda);      // :130-146
            tempChi = g2o.activeRobustChi2();                  // :148-157
            if (!ok2) tempChi = std::numeric_limits<double>::max();
            float sE, nsE;
            g2o.pointEstimates(pts);
            if ((int)pts.size() != 3 * mNV) { mStatus = ORBX_ERR_ARG; return Fail; }
            tempChi = Hook(pts, qmax, tempChi, currentChi, sE, nsE);   // :159-199
            if (mStatus != ORBX_OK) return Fail;
            rho = (currentChi - tempChi);                      // :201
            double scale = g2o.computeScale(mLambda);
            scale += 1e-3;
            rho /= scale;
            const bool good = rho > 0 && std::isfinite(tempChi);
            if (good) {                                        // :207-217
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = (std::min)(alpha, mGoodStepUpperScale);
                const double scaleFactor = (std::max)(mGoodStepLowerScale, alpha);
                mLambda *= scaleFactor;
                mNi = 2;
                currentChi = tempChi;
                g2o.discardTop();
            } else {                                           // :218-223
                mLambda *= mNi;
                mNi *= 2;
                g2o.pop();
            }
            if (log) log->push_back(Trial{sE, nsE, tempChi, currentChi, rho, mLambda, qmax, good ? 1 : 0});
            qmax++;
        } while (rho < 0 && qmax < mMaxTrialsAfterFailure && !g2o.terminate());   // :226
        if (qmax == mMaxTrialsAfterFailure || rho == 0) return Terminate;           // :228-229
        if ((iniChi - currentChi) * 1e3 < iniChi) mNBad++;                           // :232-235 (the stop criterion added in ORB-SLAM2's g2o)
        else mNBad = 0;
        if (mNBad >= 3) return Terminate;
        return OK;
    }

    // The four rounds of Optimizer.cc:733-790: its[] = {10, 10, 10, 10}; SparseOptimizer::optimize's loop stops at the
    // first result that is not OK.  Returns the number of Levenberg iterations run.
    template <class Problem>
    int Optimize(Problem &g2o, std::vector<Trial> *log = nullptr, std::vector<int> *results = nullptr)
    {
        static const int its[4] = {10, 10, 10, 10};            // :730
        int total = 0;
        for (int round = 0; round < 4; ++round) {
            g2o.initializeOptimization(round);                 // :738
            for (int i = 0; i < its[round] && !g2o.terminate(); ++i) {
                const SolverResult r = Iteration(g2o, i, log);
                ++total;
                if (results) results->push_back((int)r);
                if (r != OK) break;
            }
            g2o.classifyOutliers(round);                       // :752-790
        }
        return total;
    }

    FEA2 fea2;
    int status() const { return mStatus == ORBX_OK ? fea2.status() : mStatus; }
    double lambda() const { return mLambda; }

private:
    int mStatus = ORBX_OK, mNV = 0;
    double mLambda = -1., mNi = 2., mGoodStepLowerScale = 1. / 3., mGoodStepUpperScale = 2. / 3.;   // levenberg.cpp:48-56
    int mNBad = 0, mMaxTrialsAfterFailure = 10;                                                     // :50
};

// Optimizer::PoseOptimizationNR (src/Optimizer.cc:478-834) with the bundle itself on the device: Compute() is
// PoseOptimizationNR_fem::Compute (fea2.Compute(1)'s numeric half and the hook's state parked on the device); operator() runs
// :733-809 -- the four rounds of optimize(10), g2o's Levenberg trials with the hook, the Schur step, the inlier / outlier passes,
// the write-back -- as ONE launch of orbm_pose_optimization_nr on the graph the caller has flattened from its walk over
// MapPoint* / KeyFrame* (:515-709; integration/Optimizer_pose_nr_hip.cc).  Tcw = pFrame->mTcw (replaced by what SetPose receives),
// points = GetWorldPos() of vpMapPoints (replaced by what SetWorldPos receives), outlier = mvbOutlier by point.  Returns
// nInitialCorrespondences - nBad, or -1 on a library error (status() has the code: ORBX_ERR_UNSUPPORTED beyond the kernel's limits,
// where PoseOptimizationNR_fem with g2o's own loop remains the path).
class PoseOptimizationNR {
public:
    struct Graph {
        std::vector<float> kfTcw;                 // [nkf][16]
        std::vector<int32_t> ePoint, eCam;        // per edge, in vpEdges order; eCam -1 = the frame
        std::vector<float> eObs, eInvSigma2, eCamK;   // [ne][2], [ne], [ne][4] = fx fy cx cy
    };

    explicit PoseOptimizationNR(int nElType) : fea2(3500, 0.495f, 0.5f, 0.577350269f, nElType) {}

    bool Compute(const std::vector<float> &topXYZ, const std::vector<int32_t> &faces, int nVertices,
                 const std::vector<int32_t> &derived = std::vector<int32_t>())
    {
        if (!fea2.Compute(topXYZ, faces)) return false;
        mStatus = fem_trial_setup(fea2.model(), fea2.u0.data(), fea2.vDir.data(), (int)fea2.vDir.size(), 100000000.0f, nVertices,
                                  derived.empty() ? nullptr : derived.data(), (int)derived.size() / 4);
        return mStatus == ORBX_OK;
    }

    int operator()(const Graph &g, float Tcw[16], std::vector<float> &points, std::vector<uint8_t> &outlier,
                   orbm_pose_nr_stats *stats = nullptr)
    {
        const size_t ne = g.ePoint.size();
        if (points.size() % 3 || g.kfTcw.size() % 16 || g.eCam.size() != ne || g.eObs.size() != 2 * ne || g.eInvSigma2.size() != ne ||
            g.eCamK.size() != 4 * ne) { mStatus = ORBX_ERR_ARG; return -1; }
        orbm_pose_nr_graph c;
        std::memset(&c, 0, sizeof(c));
        c.npoints = (int32_t)(points.size() / 3); c.nkf = (int32_t)(g.kfTcw.size() / 16); c.nedges = (int32_t)ne;
        c.Tcw = Tcw; c.kf_Tcw = g.kfTcw.data(); c.points = points.data(); c.e_point = g.ePoint.data(); c.e_cam = g.eCam.data();
        c.e_obs = g.eObs.data(); c.e_inv_sigma2 = g.eInvSigma2.data(); c.e_cam_k = g.eCamK.data();
        std::vector<float> pointsOut(points.size());
        outlier.assign(points.size() / 3, 0);
        orbm_pose_nr_result r;
        std::memset(&r, 0, sizeof(r));
        r.points_out = pointsOut.data(); r.outlier = outlier.data();
        mStatus = orbm_pose_optimization_nr(fea2.model(), &c, &r, stats);
        if (mStatus != ORBX_OK) return -1;
        std::memcpy(Tcw, r.Tcw, sizeof(r.Tcw));
        points.swap(pointsOut);
        return r.ngood;
    }

    FEA2 fea2;
    int status() const { return mStatus == ORBX_OK ? fea2.status() : mStatus; }

private:
    int mStatus = ORBX_OK;
};

// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:837-1162) and Optimizer::BundleAdjustment (:74-262) over orbm_bundle_adjustment:
// a builder for the flat graph the caller fills from its walk over KeyFrame* / MapPoint* (integration/Optimizer_ba_hip.cc) and the
// call.  Keyframes: addKeyFrame for the local ones in lLocalKeyFrames order (fixed = mnId == 0), then addFixedKeyFrame; points in
// ascending index with their observations in the observations map's order.  Local() / Global() run the two protocols; poses / points
// are replaced by what SetPose / SetWorldPos receive, erase[e] = the edge is in vToErase, notIncluded[n] = the point had no edge.
// false on a library error (status(): ORBX_ERR_UNSUPPORTED beyond 64 free keyframes, where g2o remains the path).  GlobalMap() is
// Global() over orbm_global_bundle_adjustment: a whole map of up to 512 keyframes (Optimizer::GlobalBundleAdjustemnt behind a loop
// closure), the reduced system solved by the tiled multi-workgroup Cholesky; the same bytes as Global() where both accept the graph.
// GlobalMapEnv() is the same call through orbm_global_bundle_adjustment_env, for the map of a long session of up to 4,096 keyframes:
// add the keyframes by ascending mnId, since their order decides the tile envelope of the reduced system (ORBX_ERR_UNSUPPORTED beyond
// its limits, where g2o remains the path); the same numbers as GlobalMap() where both accept the graph.
class BundleAdjustment {
public:
    std::vector<float> poses, points;               // [nfree + nfixed][16], [npoints][3]
    std::vector<uint8_t> fixed;                     // [nfree]
    std::vector<int32_t> ePoint, eCam;
    std::vector<float> eObs, eInvSigma2, eCamK;     // [ne][3] (ur < 0: monocular), [ne], [ne][5] = fx fy cx cy bf
    std::vector<uint8_t> erase, notIncluded;
    int stopped = 0;

    int addKeyFrame(const float Tcw[16], bool isFixed = false)
    {
        if (nFixed) return -1;                      // the local keyframes come first
        poses.insert(poses.end(), Tcw, Tcw + 16); fixed.push_back(isFixed ? 1 : 0);
        return nFree++;
    }
    int addFixedKeyFrame(const float Tcw[16])
    {
        poses.insert(poses.end(), Tcw, Tcw + 16);
        return nFree + nFixed++;
    }
    int addPoint(const float X[3])
    {
        points.insert(points.end(), X, X + 3);
        return (int)(points.size() / 3) - 1;
    }
    // an observation of the LAST added point
    void addObservation(int keyframe, float u, float v, float ur, float invSigma2, float fx, float fy, float cx, float cy, float bf)
    {
        ePoint.push_back((int32_t)(points.size() / 3) - 1); eCam.push_back(keyframe);
        eObs.push_back(u); eObs.push_back(v); eObs.push_back(ur); eInvSigma2.push_back(invSigma2);
        const float k[5] = {fx, fy, cx, cy, bf};
        eCamK.insert(eCamK.end(), k, k + 5);
    }

    bool Local(const volatile uint8_t *pbStopFlag = nullptr, orbm_ba_stats *stats = nullptr)
    {
        const orbm_ba_options o = ORBM_BA_OPTIONS_LOCAL;
        return run(o, pbStopFlag, stats);
    }
    bool Global(int nIterations, bool bRobust, const volatile uint8_t *pbStopFlag = nullptr, orbm_ba_stats *stats = nullptr)
    {
        const orbm_ba_options o = ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust);
        return run(o, pbStopFlag, stats);
    }
    bool GlobalMap(int nIterations, bool bRobust, const volatile uint8_t *pbStopFlag = nullptr, orbm_ba_stats *stats = nullptr)
    {
        const orbm_ba_options o = ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust);
        return run(o, pbStopFlag, stats, 1);
    }
    bool GlobalMapEnv(int nIterations, bool bRobust, const volatile uint8_t *pbStopFlag = nullptr, orbm_ba_stats *stats = nullptr)
    {
        const orbm_ba_options o = ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust);
        return run(o, pbStopFlag, stats, 2);
    }
    int status() const { return mStatus; }
    int nFreeKeyFrames() const { return nFree; }

private:
    bool run(const orbm_ba_options &o, const volatile uint8_t *pbStopFlag, orbm_ba_stats *stats, int entry = 0)
    {
        orbm_ba_graph g;
        std::memset(&g, 0, sizeof(g));
        g.nfree = nFree; g.nfixed = nFixed; g.npoints = (int32_t)(points.size() / 3); g.nedges = (int32_t)ePoint.size();
        g.poses = poses.data(); g.fixed = fixed.data(); g.points = points.data(); g.e_point = ePoint.data(); g.e_cam = eCam.data();
        g.e_obs = eObs.data(); g.e_inv_sigma2 = eInvSigma2.data(); g.e_cam_k = eCamK.data();
        std::vector<float> posesOut(16 * (size_t)nFree + 1), pointsOut(points.size() + 1);
        erase.assign(ePoint.size() + 1, 0); notIncluded.assign(points.size() / 3 + 1, 0);
        orbm_ba_result r;
        std::memset(&r, 0, sizeof(r));
        r.poses = posesOut.data(); r.points = pointsOut.data(); r.erase = erase.data(); r.not_included = notIncluded.data();
        mStatus = entry == 2   ? orbm_global_bundle_adjustment_env(&g, &o, pbStopFlag, &r, stats)
                  : entry == 1 ? orbm_global_bundle_adjustment(&g, &o, pbStopFlag, &r, stats)
                               : orbm_bundle_adjustment(&g, &o, pbStopFlag, &r, stats);
        if (mStatus != ORBX_OK) return false;
        std::copy(posesOut.begin(), posesOut.begin() + 16 * (size_t)nFree, poses.begin());
        std::copy(pointsOut.begin(), pointsOut.begin() + points.size(), points.begin());
        erase.resize(ePoint.size()); notIncluded.resize(points.size() / 3);
        stopped = r.stopped;
        return true;
    }
    int nFree = 0, nFixed = 0, mStatus = ORBX_OK;
};

// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1165-1428) over orbm_essential_graph: a builder for the flat graph the caller
// fills from its walk (integration/Optimizer_essential_graph_hip.cc) and the call.  addKeyFrame in vpKFs order (corrected /
// nonCorrected: the CorrectedSim3 / NonCorrectedSim3 entry as q xyzw, t, s, or nullptr); the edges in the reference's creation order:
// addLoopConnection for the LoopConnections loop (:1236-1264), addEdge for a spanning-tree, old-loop or covisibility edge
// (:1284-1366), vertex 0 = nIDi first; addPoint with the index of the keyframe :1404-1413 choose.  Optimize() replaces poses by what
// SetPose receives and points by what SetWorldPos receives.  false on a library error (status(): ORBX_ERR_UNSUPPORTED beyond 438
// free keyframes with an edge).  OptimizeEnv() is the same call through orbm_essential_graph_env, for up to 4,096 free keyframes: add
// the keyframes by ascending mnId, since their order decides the tile envelope (ORBX_ERR_UNSUPPORTED beyond its limits, where g2o
// remains the path).
class EssentialGraph {
public:
    std::vector<float> poses, points;               // [nvert][16], [npoints][3]
    std::vector<int32_t> corrected, nonCorrected;   // [nvert]: row of the table, or -1
    std::vector<double> correctedSim3, nonCorrectedSim3;    // [..][8]
    std::vector<uint8_t> fixed, eKind;
    std::vector<int32_t> eV0, eV1, pRef;
    bool fixScale = true;

    int addKeyFrame(const float Tcw[16], bool isFixed = false, const double *correctedEntry = nullptr, const double *nonCorrectedEntry = nullptr)
    {
        poses.insert(poses.end(), Tcw, Tcw + 16); fixed.push_back(isFixed ? 1 : 0);
        corrected.push_back(entry(correctedSim3, correctedEntry)); nonCorrected.push_back(entry(nonCorrectedSim3, nonCorrectedEntry));
        return (int)fixed.size() - 1;
    }
    void addLoopConnection(int vi, int vj) { eV0.push_back(vi); eV1.push_back(vj); eKind.push_back(0); }
    void addEdge(int vi, int vj) { eV0.push_back(vi); eV1.push_back(vj); eKind.push_back(1); }
    int addPoint(const float X[3], int reference)
    {
        points.insert(points.end(), X, X + 3); pRef.push_back(reference);
        return (int)pRef.size() - 1;
    }

    bool Optimize(int nIterations = ORBM_EG_ITERATIONS, orbm_eg_stats *stats = nullptr) { return run(orbm_essential_graph, nIterations, stats); }
    bool OptimizeEnv(int nIterations = ORBM_EG_ITERATIONS, orbm_eg_stats *stats = nullptr) { return run(orbm_essential_graph_env, nIterations, stats); }
    int status() const { return mStatus; }

private:
    bool run(int (*call)(const orbm_eg_graph *, const orbm_eg_options *, orbm_eg_result *, orbm_eg_stats *), int nIterations, orbm_eg_stats *stats)
    {
        orbm_eg_graph g;
        std::memset(&g, 0, sizeof(g));
        g.nvert = (int32_t)fixed.size(); g.ncorr = (int32_t)(correctedSim3.size() / 8); g.nnc = (int32_t)(nonCorrectedSim3.size() / 8);
        g.nedges = (int32_t)eV0.size(); g.npoints = (int32_t)pRef.size(); g.fix_scale = fixScale ? 1 : 0;
        g.poses = poses.data(); g.corrected = corrected.data(); g.corrected_sim3 = correctedSim3.data(); g.noncorrected = nonCorrected.data();
        g.noncorrected_sim3 = nonCorrectedSim3.data(); g.fixed = fixed.data(); g.e_v0 = eV0.data(); g.e_v1 = eV1.data(); g.e_kind = eKind.data();
        g.points = points.data(); g.p_ref = pRef.data();
        orbm_eg_options o = ORBM_EG_OPTIONS_DEFAULT;
        o.iterations = nIterations;
        std::vector<float> posesOut(poses.size() + 1), pointsOut(points.size() + 1);
        orbm_eg_result r;
        r.poses = posesOut.data(); r.points = pointsOut.data();
        mStatus = call(&g, &o, &r, stats);
        if (mStatus != ORBX_OK) return false;
        std::copy(posesOut.begin(), posesOut.begin() + poses.size(), poses.begin());
        std::copy(pointsOut.begin(), pointsOut.begin() + points.size(), points.begin());
        return true;
    }
    static int32_t entry(std::vector<double> &table, const double *e)
    {
        if (!e) return -1;
        table.insert(table.end(), e, e + 8);
        return (int32_t)(table.size() / 8) - 1;
    }
    int mStatus = ORBX_OK;
};

// Optimizer::PoseOptimization(Frame *pFrame) (src/Optimizer.cc:264-476) on the flattened frame: one call of
// orbm_pose_optimization (host arrays) or orbm_frame_pose_optimization (the frame's resident handle).  kpsUn = mvKeysUn,
// uright = mvuRight (empty: monocular), hasMp[i] = mvpMapPoints[i] != NULL, mpPos[3 i ..] = its GetWorldPos(), Tcw = mTcw
// (4 x 4 row-major floats, replaced by the optimised pose as SetPose would), outlier = mvbOutlier (written where hasMp).
// Returns nInitialCorrespondences - nBad, or -1 on a library error (status() has the code).
class PoseOptimization {
public:
    PoseOptimization(float fx, float fy, float cx, float cy, float mbf, std::vector<float> invLevelSigma2)
        : mInv(std::move(invLevelSigma2))
    {
        mCam.fx = fx; mCam.fy = fy; mCam.cx = cx; mCam.cy = cy; mCam.bf = mbf;
        mCam.nlevels = (int32_t)mInv.size();
        mCam.inv_level_sigma2 = mInv.data();
    }
    PoseOptimization(const PoseOptimization &) = delete;
    PoseOptimization &operator=(const PoseOptimization &) = delete;

    int operator()(const std::vector<orbx_keypoint> &kpsUn, const std::vector<float> &uright, const std::vector<uint8_t> &hasMp,
                   const std::vector<float> &mpPos, float Tcw[16], std::vector<uint8_t> &outlier, orbm_pose_stats *stats = nullptr)
    {
        const int n = (int)kpsUn.size();
        if ((int)hasMp.size() != n || (int)mpPos.size() != 3 * n || (!uright.empty() && (int)uright.size() != n)) return fail(ORBX_ERR_ARG);
        outlier.resize(n, 0);
        float Tout[16];
        int ngood = 0;
        mStatus = orbm_pose_optimization(kpsUn.data(), uright.empty() ? nullptr : uright.data(), n, hasMp.data(), mpPos.data(), &mCam, Tcw,
                                         Tout, outlier.data(), &ngood, stats);
        if (mStatus != ORBX_OK) return -1;
        std::memcpy(Tcw, Tout, sizeof(Tout));
        return ngood;
    }
    int operator()(const orbm_frame *frame, const std::vector<uint8_t> &hasMp, const std::vector<float> &mpPos, float Tcw[16],
                   std::vector<uint8_t> &outlier, orbm_pose_stats *stats = nullptr)
    {
        if (mpPos.size() != 3 * hasMp.size()) return fail(ORBX_ERR_ARG);
        outlier.resize(hasMp.size(), 0);
        float Tout[16];
        int ngood = 0;
        mStatus = orbm_frame_pose_optimization(frame, hasMp.data(), mpPos.data(), &mCam, Tcw, Tout, outlier.data(), &ngood, stats);
        if (mStatus != ORBX_OK) return -1;
        std::memcpy(Tcw, Tout, sizeof(Tout));
        return ngood;
    }
    int status() const { return mStatus; }

private:
    int fail(int code) { mStatus = code; return -1; }
    std::vector<float> mInv;
    orbm_pose_camera mCam;
    int mStatus = ORBX_OK;
};

// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over orbm_sim3_hypotheses.  The constructor takes the flat problem -- what
// the reference's constructor keeps of the two keyframes (:62-103): world positions and keypoint octaves of the kept pairs, where
// each pair stands in vpMatched12 (indices1 = mvnIndices1, N1 = vpMatched12.size()), the two poses and calibrations -- and a
// source of draws: a callback int(int lo, int hi) (inclusive, as DUtils::Random::RandomInt) or pre-drawn triples.  The first
// iterate() draws the triples of all mRansacMaxIts iterations in the reference's order (:163-177) and evaluates them in one
// orbm_sim3_hypotheses call; every iterate() is then the reference's fold (:158-206) over the stored inlier counts, with no device
// work.  EvaluateBatch does the first evaluation of all candidates of a loop detection in one call.
// One difference to the reference: the draws of one solver are made together; in LoopClosing::ComputeSim3 they interleave with the
// other candidates' draws in five-iteration rounds.  Results equal the reference run whose RNG hands each solver these triples
// (the reference seeds nothing here).  iterate() returns true and fills T12 where the reference returns a non-empty matrix.
class Sim3Solver {
public:
    struct Problem {
        std::vector<float> X1w, X2w;            // [n][3]
        std::vector<int32_t> octave1, octave2;  // [n]
        std::vector<int32_t> indices1;          // [n] mvnIndices1; empty: 0 .. n-1
        int N1 = -1;                            // vpMatched12.size(); -1: n
        float Tcw1[16], Tcw2[16];
        float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
        std::vector<float> levelSigma2;         // mvLevelSigma2
        bool bFixScale = false;
    };
    typedef int (*DrawFn)(int lo, int hi);

    Sim3Solver(Problem problem, DrawFn draw) : mP(std::move(problem)), mDraw(draw) { init(); }
    Sim3Solver(Problem problem, std::vector<int32_t> triples) : mP(std::move(problem)), mDraw(nullptr), mTriples(std::move(triples)) { init(); }
    Sim3Solver(const Sim3Solver &) = delete;
    Sim3Solver &operator=(const Sim3Solver &) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability; mRansacMinInliers = minInliers; mRansacMaxIts = maxIterations;
        const float epsilon = (float)mRansacMinInliers / N;                                  // :125
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : std::numeric_limits<int>::min();   // what x86 makes of it
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
    }

    // The first evaluation of every solver that has not had it (and has N >= mRansacMinInliers), at most 64 per launch.
    static int EvaluateBatch(const std::vector<Sim3Solver *> &solvers)
    {
        std::vector<Sim3Solver *> todo;
        for (Sim3Solver *s : solvers) if (s && !s->mEvaluated && s->N >= s->mRansacMinInliers) todo.push_back(s);
        int rc = ORBX_OK;
        for (size_t b = 0; b < todo.size() && rc == ORBX_OK; b += 64) {
            const size_t e = std::min(todo.size(), b + 64);
            std::vector<orbm_sim3_problem> probs;
            size_t total = 0, words = 0;
            for (size_t k = b; k < e; ++k) {
                Sim3Solver &s = *todo[k];
                if ((rc = s.draw()) != ORBX_OK) break;
                const Problem &p = s.mP;
                orbm_sim3_problem q;
                q.X1w = p.X1w.data(); q.X2w = p.X2w.data(); q.octave1 = p.octave1.data(); q.octave2 = p.octave2.data();
                q.Tcw1 = p.Tcw1; q.Tcw2 = p.Tcw2;
                q.fx1 = p.fx1; q.fy1 = p.fy1; q.cx1 = p.cx1; q.cy1 = p.cy1; q.fx2 = p.fx2; q.fy2 = p.fy2; q.cx2 = p.cx2; q.cy2 = p.cy2;
                q.triples = s.mTriples.data(); q.n = s.N; q.H = s.mRansacMaxIts; q.fix_scale = p.bFixScale ? 1 : 0;
                probs.push_back(q);
                total += (size_t)q.H; words += (size_t)q.H * (size_t)((q.n + 63) / 64);
            }
            if (rc != ORBX_OK) break;
            std::vector<orbm_sim3_hypothesis> hyp(total ? total : 1);
            std::vector<uint64_t> masks(words ? words : 1);
            const std::vector<float> &sg = todo[b]->mP.levelSigma2;
            rc = orbm_sim3_hypotheses(probs.data(), (int)probs.size(), sg.data(), (int)sg.size(), hyp.data(), masks.data());
            size_t h0 = 0, w0 = 0;
            for (size_t k = b; k < e; ++k) {
                Sim3Solver &s = *todo[k];
                s.mStatus = rc;
                const size_t H = (size_t)s.mRansacMaxIts, W = H * (size_t)((s.N + 63) / 64);
                if (rc == ORBX_OK) {
                    s.mHyp.assign(hyp.begin() + h0, hyp.begin() + h0 + H);
                    s.mMasks.assign(masks.begin() + w0, masks.begin() + w0 + W);
                    s.mEvaluated = true;
                }
                h0 += H; w0 += W;
            }
        }
        return rc;
    }

    // iterate (:140-207).  T12: 4 x 4 row-major, written when the result is true.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float T12[16])
    {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) { bNoMore = true; return false; }
        if (!mEvaluated) {
            std::vector<Sim3Solver *> one(1, this);
            if (EvaluateBatch(one) != ORBX_OK) { bNoMore = true; return false; }      // status() has the code
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            const int h = mnIterations;
            nCurrentIterations++;
            mnIterations++;
            const int cnt = mHyp[h].ninliers;
            if (cnt >= mnBestInliers) {
                mnBestInliers = cnt; mBest = h;
                if (cnt > mRansacMinInliers) {
                    nInliers = cnt;
                    const int W = (N + 63) / 64;
                    for (int i = 0; i < N; i++)
                        if ((mMasks[(size_t)h * W + i / 64] >> (i % 64)) & 1u) vbInliers[mP.indices1.empty() ? i : mP.indices1[i]] = true;
                    std::memcpy(T12, mHyp[h].T12, sizeof(float) * 16);
                    return true;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return false;
    }

    bool find(std::vector<bool> &vbInliers12, int &nInliers, float T12[16])
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
    }

    // mBestRotation (3 x 3 row-major), mBestTranslation, mBestScale; false before any hypothesis was held as best
    bool GetEstimatedRotation(float R[9]) const { if (mBest < 0) return false; std::memcpy(R, mHyp[mBest].R12, sizeof(float) * 9); return true; }
    bool GetEstimatedTranslation(float t[3]) const { if (mBest < 0) return false; std::memcpy(t, mHyp[mBest].t12, sizeof(float) * 3); return true; }
    float GetEstimatedScale() const { return mBest < 0 ? 0.f : mHyp[mBest].s12; }
    int GetRansacMaxIts() const { return mRansacMaxIts; }
    int status() const { return mStatus; }

private:
    void init()
    {
        N = (int)(mP.X1w.size() / 3);
        mN1 = mP.N1 < 0 ? N : mP.N1;
        SetRansacParameters();
    }
    int draw()      // the draw loop of :163-177 for all mRansacMaxIts iterations
    {
        const size_t need = 3 * (size_t)mRansacMaxIts;
        if (!mDraw) return mTriples.size() >= need ? ORBX_OK : (mStatus = ORBX_ERR_ARG);
        if (N < 3) return mStatus = ORBX_ERR_ARG;
        mTriples.resize(need);
        std::vector<int32_t> avail;
        for (int h = 0; h < mRansacMaxIts; ++h) {
            avail.resize((size_t)N);
            for (int i = 0; i < N; ++i) avail[i] = i;
            for (int i = 0; i < 3; ++i) {
                const int randi = mDraw(0, (int)avail.size() - 1);
                if (randi < 0 || randi >= (int)avail.size()) return mStatus = ORBX_ERR_ARG;
                mTriples[3 * (size_t)h + i] = avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
        }
        return ORBX_OK;
    }
    Problem mP;
    DrawFn mDraw;
    std::vector<int32_t> mTriples;
    std::vector<orbm_sim3_hypothesis> mHyp;
    std::vector<uint64_t> mMasks;
    double mRansacProb = 0.99;
    int N = 0, mN1 = 0, mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0, mBest = -1, mStatus = ORBX_OK;
    bool mEvaluated = false;
};

// PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) over orbm_pnp_hypotheses.  The constructor takes the flat problem -- what the
// reference's constructor keeps of the frame (:81-103): world positions, undistorted pixels and keypoint octaves of the kept
// matches, where each stands in vpMapPointMatches (indices = mvKeyPointIndices, nMatches = vpMapPointMatches.size()), the
// calibration -- and a source of draws: a callback int(int lo, int hi) (inclusive, as DUtils::Random::RandomInt) or pre-drawn
// sets, consumed in order.  An iterate() draws the sets of every iteration it can run, in the reference's order (:193-206),
// evaluates them in one orbm_pnp_hypotheses call with the carried mnBestInliers (compute_pose, CheckInliers and the Refine behind
// every new best), and is then the reference's fold (:187-262) over the results.  The first iterate(5) runs every iteration up to
// mRansacMaxIts (the loop condition of :187 is an OR); each later call runs nIterations more.  evaluate() does that evaluation for
// all candidates of a relocalisation in one call.
// One difference to the reference: the draws of one solver are made together; in Tracking::Relocalization they interleave with the
// other candidates' draws in five-iteration rounds.  Results equal the reference run whose RNG hands each solver these sets (the
// reference seeds nothing here), with the arithmetic of DESIGN 22.  iterate() returns true and fills Tcw where the reference
// returns a non-empty matrix.
class PnPsolver {
public:
    struct Problem {
        std::vector<float> Xw, uv;              // [n][3] mvP3Dw, [n][2] mvP2D
        std::vector<int32_t> octave;            // [n]
        std::vector<int32_t> indices;           // [n] mvKeyPointIndices; empty: 0 .. n-1
        int nMatches = -1;                      // vpMapPointMatches.size(); -1: n
        double fu = 0, fv = 0, uc = 0, vc = 0;
        std::vector<float> levelSigma2;         // mvLevelSigma2
    };
    struct RecordedPose { double R[9], t[3]; int nInliers, iteration; };      // RPoses / tPoses [iteration], inlierPoses of the fork's first stage
    typedef int (*DrawFn)(int lo, int hi);
    typedef bool (*AcceptFn)(const double R[9], const double t[3], void *user);

    PnPsolver(Problem problem, DrawFn draw) : mP(std::move(problem)), mDraw(draw) { init(); }
    PnPsolver(Problem problem, std::vector<int32_t> sets) : mP(std::move(problem)), mDraw(nullptr), mSets(std::move(sets)) { init(); }
    PnPsolver(const PnPsolver &) = delete;
    PnPsolver &operator=(const PnPsolver &) = delete;

    // :123-159
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                             float th2 = 5.991f)
    {
        mRansacProb = probability; mRansacMinInliers = minInliers; mRansacMaxIts = maxIterations; mRansacEpsilon = epsilon;
        mRansacMinSet = minSet; mTh2 = th2;
        int nMinInliers = (int)(N * mRansacEpsilon);
        if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(mRansacEpsilon, 3)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : std::numeric_limits<int>::min();   // what x86 makes of it
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mHyp.clear();                           // min_inliers decides the records: evaluate again
    }

    // The evaluation that each solver's next iterate(nIterations) needs, at most 64 solvers per launch.
    static int evaluate(const std::vector<PnPsolver *> &solvers, int nIterations = 5)
    {
        std::vector<PnPsolver *> todo;
        for (PnPsolver *s : solvers) {
            if (!s || s->N < s->mRansacMinInliers || s->mRansacMinSet != 4) continue;
            const int a = s->mnIterations, b = a + s->span(nIterations);
            if (b > a && !s->covered(a, b)) todo.push_back(s);
        }
        int rc = ORBX_OK;
        for (size_t b0 = 0; b0 < todo.size() && rc == ORBX_OK; b0 += 64) {
            const size_t e = std::min(todo.size(), b0 + 64);
            std::vector<orbm_pnp_problem> probs;
            std::vector<int32_t> best;
            size_t total = 0, words = 0;
            for (size_t k = b0; k < e; ++k) {
                PnPsolver &s = *todo[k];
                const int a = s.mnIterations, b = a + s.span(nIterations);
                if ((rc = s.draw(b, false)) != ORBX_OK) break;
                probs.push_back(s.problem(a, b));
                best.push_back(s.mnBestInliers);
                total += (size_t)(b - a); words += (size_t)(b - a) * (size_t)((s.N + 63) / 64);
            }
            if (rc != ORBX_OK) break;
            std::vector<orbm_pnp_hypothesis> hyp(total ? total : 1);
            std::vector<uint64_t> masks(words ? words : 1), rmasks(words ? words : 1);
            const std::vector<float> &sg = todo[b0]->mP.levelSigma2;
            rc = orbm_pnp_hypotheses(probs.data(), (int)probs.size(), sg.data(), (int)sg.size(), best.data(), hyp.data(), masks.data(), rmasks.data());
            size_t h0 = 0, w0 = 0;
            for (size_t k = b0; k < e; ++k) {
                PnPsolver &s = *todo[k];
                s.mStatus = rc;
                const size_t H = (size_t)probs[k - b0].H, W = H * (size_t)((s.N + 63) / 64);
                if (rc == ORBX_OK) s.store(s.mnIterations, hyp.data() + h0, masks.data() + w0, rmasks.data() + w0, H, W);
                h0 += H; w0 += W;
            }
        }
        return rc;
    }

    // iterate (:170-263).  Tcw: 4 x 4 row-major, written when the result is true.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float Tcw[16])
    {
        bNoMore = false;
        vbInliers = std::vector<bool>(mNMatches, false);
        nInliers = 0;
        if (N < mRansacMinInliers) { bNoMore = true; return false; }
        {
            std::vector<PnPsolver *> one(1, this);
            if (evaluate(one, nIterations) != ORBX_OK || mStatus != ORBX_OK) { bNoMore = true; return false; }      // status() has the code
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
            const int k = mnIterations - mStart;
            nCurrentIterations++;
            mnIterations++;
            if (consider(k) && mnRefinedInliers > mRansacMinInliers) {      // Refine() (:681)
                nInliers = mnRefinedInliers;
                scatter(mRefinedMask, vbInliers);
                toTcw(mRefinedR, mRefinedt, Tcw);
                return true;
            }
        }
        if (mnIterations >= mRansacMaxIts) {
            bNoMore = true;
            if (mnBestInliers >= mRansacMinInliers && !mBestMask.empty()) {
                nInliers = mnBestInliers;
                scatter(mBestMask, vbInliers);
                toTcw(mBestR, mBestt, Tcw);
                return true;
            }
        }
        return false;
    }

    bool find(std::vector<bool> &vbInliers, int &nInliers, float Tcw[16])
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers, Tcw);
    }

    // The first stage of iterate(Frame &, .., Map *) (:267-416) as a fold over one evaluation: mnIterations restarts at 0, the sets
    // are drawn with that function's own erase rule (:315 overwrites element [idx], not [randi], so a set may repeat a
    // correspondence), every pose with 2 < inliers < mRansacMinInliers is recorded for the second stage, and accept(R, t, user) --
    // the caller's whole-map SearchByProjection under the refined pose, true for nMatched >= 12 -- decides a successful Refine.
    // Refines behind the accepted one are speculative: computed in the same call and never read.
    bool iterateFrameStage1(int nIterations, AcceptFn accept, void *user, std::vector<bool> &vbInliers, int &nInliers, float Tcw[16],
                            std::vector<RecordedPose> &poses)
    {
        vbInliers = std::vector<bool>(mNMatches, false);
        nInliers = 0;
        poses.clear();
        mnIterations = 0;
        if (mDraw) mSets.clear();
        const int total = std::max(mRansacMaxIts, nIterations);
        if ((mStatus = draw(total, true)) != ORBX_OK) return false;
        const orbm_pnp_problem q = problem(0, total);
        std::vector<orbm_pnp_hypothesis> hyp((size_t)total);
        const size_t W = (size_t)total * (size_t)((N + 63) / 64);
        std::vector<uint64_t> masks(W ? W : 1), rmasks(W ? W : 1);
        const int32_t best = mnBestInliers;
        mStatus = orbm_pnp_hypotheses(&q, 1, mP.levelSigma2.data(), (int)mP.levelSigma2.size(), &best, hyp.data(), masks.data(), rmasks.data());
        if (mStatus != ORBX_OK) return false;
        store(0, hyp.data(), masks.data(), rmasks.data(), (size_t)total, W);
        int verdict = -1;
        for (int k = 0; k < total; ++k) {
            mnIterations++;
            const orbm_pnp_hypothesis &h = mHyp[k];
            if (h.ninliers > 2 && h.ninliers < mRansacMinInliers) {
                RecordedPose p;
                std::memcpy(p.R, h.R, sizeof(p.R)); std::memcpy(p.t, h.t, sizeof(p.t)); p.nInliers = h.ninliers; p.iteration = k;
                poses.push_back(p);
            }
            const int before = mnBestInliers;
            if (consider(k) && mnRefinedInliers > mRansacMinInliers) {
                if (mnBestInliers != before) verdict = -1;                  // the same pose gives the same search
                if (verdict < 0) verdict = accept(mRefinedR, mRefinedt, user) ? 1 : 0;
                if (verdict == 1) {
                    nInliers = mnRefinedInliers;
                    scatter(mRefinedMask, vbInliers);
                    toTcw(mRefinedR, mRefinedt, Tcw);
                    return true;
                }
            }
        }
        return false;
    }

    int GetRansacMaxIts() const { return mRansacMaxIts; }
    int GetRansacMinInliers() const { return mRansacMinInliers; }
    float GetRansacEpsilon() const { return mRansacEpsilon; }
    int GetIterations() const { return mnIterations; }
    int GetBestInliers() const { return mnBestInliers; }
    int status() const { return mStatus; }

private:
    void init()
    {
        N = (int)(mP.Xw.size() / 3);
        mNMatches = mP.nMatches < 0 ? N : mP.nMatches;
        SetRansacParameters();
    }
    int span(int nIterations) const { return std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0); }
    bool covered(int a, int b) const { return !mHyp.empty() && mStart <= a && b <= mStart + (int)mHyp.size(); }
    orbm_pnp_problem problem(int a, int b) const
    {
        orbm_pnp_problem q;
        q.Xw = mP.Xw.data(); q.uv = mP.uv.data(); q.octave = mP.octave.data(); q.sets = mSets.data() + 4 * (size_t)a;
        q.fu = mP.fu; q.fv = mP.fv; q.uc = mP.uc; q.vc = mP.vc; q.th2 = mTh2;
        q.n = N; q.H = b - a; q.min_inliers = mRansacMinInliers;
        return q;
    }
    void store(int start, const orbm_pnp_hypothesis *hyp, const uint64_t *masks, const uint64_t *rmasks, size_t H, size_t W)
    {
        mStart = start;
        mHyp.assign(hyp, hyp + H); mMasks.assign(masks, masks + W); mRMasks.assign(rmasks, rmasks + W);
    }
    // :214-232 for the stored hypothesis k: false below mRansacMinInliers; a new best takes its pose, flags and Refine result (a
    // record here is a record on the device: both start from the same mnBestInliers and walk the same counts); Refine() on an
    // unchanged mvbBestInliers repeats its last result
    bool consider(int k)
    {
        const orbm_pnp_hypothesis &h = mHyp[k];
        if (h.ninliers < mRansacMinInliers) return false;
        if (h.ninliers > mnBestInliers) {
            const size_t W = (size_t)((N + 63) / 64);
            mnBestInliers = h.ninliers;
            std::memcpy(mBestR, h.R, sizeof(mBestR)); std::memcpy(mBestt, h.t, sizeof(mBestt));
            mBestMask.assign(mMasks.begin() + k * W, mMasks.begin() + (k + 1) * W);
            mnRefinedInliers = h.nrefined;
            std::memcpy(mRefinedR, h.Rr, sizeof(mRefinedR)); std::memcpy(mRefinedt, h.tr, sizeof(mRefinedt));
            mRefinedMask.assign(mRMasks.begin() + k * W, mRMasks.begin() + (k + 1) * W);
        }
        return true;
    }
    void scatter(const std::vector<uint64_t> &mask, std::vector<bool> &vbInliers) const
    {
        for (int i = 0; i < N; i++)
            if ((mask[i / 64] >> (i % 64)) & 1u) vbInliers[mP.indices.empty() ? i : mP.indices[i]] = true;
    }
    static void toTcw(const double R[9], const double t[3], float Tcw[16])     // the float conversion of :223-229
    {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Tcw[4 * r + c] = (float)R[3 * r + c];
            Tcw[4 * r + 3] = (float)t[r];
            Tcw[12 + r] = 0.f;
        }
        Tcw[15] = 1.f;
    }
    int draw(int upTo, bool frameRule)      // the draw loop of :193-206 (frameRule: of :304-317) until mSets holds upTo sets
    {
        const size_t need = 4 * (size_t)upTo;
        if (mSets.size() >= need) return ORBX_OK;
        if (!mDraw || N < 4) return mStatus = ORBX_ERR_ARG;
        std::vector<int32_t> avail;
        for (int h = (int)(mSets.size() / 4); h < upTo; ++h) {
            avail.resize((size_t)N);
            for (int i = 0; i < N; ++i) avail[i] = i;
            int size = N;
            for (int i = 0; i < 4; ++i) {
                const int randi = mDraw(0, size - 1);
                if (randi < 0 || randi >= size) return mStatus = ORBX_ERR_ARG;
                const int idx = avail[randi];
                mSets.push_back(idx);
                avail[frameRule ? idx : randi] = avail[size - 1];       // (the fork's write may land behind the list's end: spare capacity)
                --size;
            }
        }
        return ORBX_OK;
    }
    Problem mP;
    DrawFn mDraw;
    std::vector<int32_t> mSets;
    std::vector<orbm_pnp_hypothesis> mHyp;
    std::vector<uint64_t> mMasks, mRMasks, mBestMask, mRefinedMask;
    double mRansacProb = 0.99, mBestR[9], mBestt[3], mRefinedR[9], mRefinedt[3];
    float mRansacEpsilon = 0.4f, mTh2 = 5.991f;
    int N = 0, mNMatches = 0, mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 4, mnIterations = 0, mnBestInliers = 0,
        mnRefinedInliers = 0, mStart = 0, mStatus = ORBX_OK;
};

// Optimizer::OptimizeSim3 (src/Optimizer.cc:1425-1625) over orbm_optimize_sim3: the caller does the pointer walk of :1483-1520 and
// passes the correspondences it keeps, flat and in that order; the whole of :1564-1624 -- both optimisation rounds, the cut between
// them and the final count -- is then ONE library call for up to 64 problems.  kept[i] of a problem says whether the reference
// leaves vpMatches1[idx] of pair i non-NULL; result.nin is the reference's return value and (q, t, s) its g2oS12 on return.
struct Sim3OptProblem {
    std::vector<float> X1w, X2w;                // [n][3] GetWorldPos() of pMP1 / pMP2
    std::vector<float> obs1, obs2;              // [n][2] mvKeysUn[i].pt, mvKeysUn[i2].pt
    std::vector<int32_t> octave1, octave2;      // [n]
    float Tcw1[16], Tcw2[16];
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float R12[9], t12[3], s12;                  // the Sim3 as LoopClosing.cc:320-325 hands it over
    float th2 = 10.f;
    bool bFixScale = false;
};

// results: one per problem; kept: one vector per problem.  invLevelSigma2 = mvInvLevelSigma2 (one pyramid).
inline int OptimizeSim3(const std::vector<Sim3OptProblem> &problems, const std::vector<float> &invLevelSigma2,
                        std::vector<orbm_sim3_opt_result> &results, std::vector<std::vector<uint8_t> > &kept)
{
    std::vector<orbm_sim3_opt_problem> flat(problems.size());
    size_t total = 0;
    for (size_t k = 0; k < problems.size(); ++k) {
        const Sim3OptProblem &p = problems[k];
        orbm_sim3_opt_problem &q = flat[k];
        const size_t n = p.octave1.size();
        if (p.X1w.size() != 3 * n || p.X2w.size() != 3 * n || p.obs1.size() != 2 * n || p.obs2.size() != 2 * n || p.octave2.size() != n) return ORBX_ERR_ARG;
        q.X1w = p.X1w.data(); q.X2w = p.X2w.data(); q.obs1 = p.obs1.data(); q.obs2 = p.obs2.data();
        q.octave1 = p.octave1.data(); q.octave2 = p.octave2.data(); q.Tcw1 = p.Tcw1; q.Tcw2 = p.Tcw2;
        q.fx1 = p.fx1; q.fy1 = p.fy1; q.cx1 = p.cx1; q.cy1 = p.cy1; q.fx2 = p.fx2; q.fy2 = p.fy2; q.cx2 = p.cx2; q.cy2 = p.cy2;
        memcpy(q.R12, p.R12, sizeof(q.R12)); memcpy(q.t12, p.t12, sizeof(q.t12));
        q.s12 = p.s12; q.th2 = p.th2; q.fix_scale = p.bFixScale ? 1 : 0; q.n = (int32_t)n;
        total += n;
    }
    results.assign(problems.size(), orbm_sim3_opt_result());
    std::vector<uint8_t> all(total ? total : 1, 0);
    const int rc = orbm_optimize_sim3(flat.data(), (int)flat.size(), invLevelSigma2.data(), (int)invLevelSigma2.size(), results.data(), all.data());
    kept.assign(problems.size(), std::vector<uint8_t>());
    if (rc != ORBX_OK) return rc;
    size_t at = 0;
    for (size_t k = 0; k < problems.size(); ++k) {
        kept[k].assign(all.begin() + at, all.begin() + at + flat[k].n);
        at += (size_t)flat[k].n;
    }
    return ORBX_OK;
}

// The refinement tail of LoopClosing::ComputeSim3 (src/LoopClosing.cc:311-341) over orbm_refine_sim3_candidates: per attempt
// SearchBySim3 chained into OptimizeSim3, pointer walk included, for every candidate whose solver returned a similarity in one pass of
// the loop at :288 -- ONE library call, one host wait.  An attempt has no side effects in the reference, so evaluating the attempts of
// a pass together and taking the first in order with nin >= 20 gives the reference's result.
struct RefineSim3Attempt {
    const ORBmatcher::ResidentFrame *KF2 = nullptr;
    const ORBmatcher::PointList *points2 = nullptr;     // one entry per keypoint of KF2: valid = map point non-NULL and not bad
    float T2w[16];
    float R12[9], t12[3], s12 = 1.f;                    // the Sim3 as LoopClosing.cc:320-325 hands it over
    std::vector<int32_t> seed12;                        // [N1] vpMapPointMatches (:313-319): >= 0 GetIndexInKeyFrame(pKF2), -1 NULL, -2 without an index; empty: all -1
    // results
    std::vector<int32_t> found12, matches12;            // what SearchBySim3 alone writes; vpMatches1 as OptimizeSim3 leaves it
    int nFound = 0;
    orbm_sim3_opt_result result;                        // result.nin = OptimizeSim3's return value, (q, t, s) = gScm on return
};

// Returns the library's status.  *accepted (optional) = the fold of the loop at :288 over this pass: the index of the first attempt in
// order with nin >= minInliers, -1 when there is none.  points1: one entry per keypoint of KF1 (mpCurrentKF).
inline int RefineSim3Candidates(const ORBmatcher::ResidentFrame &KF1, const ORBmatcher::PointList &points1, const float *T1w,
                                const ORBmatcher::Calibration &K, const std::vector<float> &invLevelSigma2,
                                std::vector<RefineSim3Attempt> &attempts, bool bFixScale, int *accepted = nullptr, float th = 7.5f,
                                float th2 = 10.f, int minInliers = 20)
{
    if (accepted) *accepted = -1;
    const size_t N1 = (size_t)KF1.N;
    const orbm_points p1 = points1.view(); const orbm_view v = K.view();
    std::vector<orbm_refine_sim3_attempt> flat(attempts.size());
    std::vector<orbm_points> p2(attempts.size());
    for (size_t k = 0; k < attempts.size(); ++k) {
        RefineSim3Attempt &a = attempts[k];
        orbm_refine_sim3_attempt &q = flat[k];
        if (!a.KF2 || !a.points2 || (!a.seed12.empty() && a.seed12.size() != N1)) return ORBX_ERR_ARG;
        p2[k] = a.points2->view();
        a.found12.assign(N1 ? N1 : 1, -1); a.matches12.assign(N1 ? N1 : 1, -1);
        q.kf2 = a.KF2->handle(); q.points2 = &p2[k]; q.T2w = a.T2w;
        memcpy(q.R12, a.R12, sizeof(q.R12)); memcpy(q.t12, a.t12, sizeof(q.t12)); q.s12 = a.s12;
        q.seed12 = a.seed12.empty() ? nullptr : a.seed12.data(); q.found12 = a.found12.data(); q.matches12 = a.matches12.data();
    }
    std::vector<int32_t> nfound(attempts.size() ? attempts.size() : 1, 0);
    std::vector<orbm_sim3_opt_result> results(attempts.size() ? attempts.size() : 1, orbm_sim3_opt_result());
    const int rc = orbm_refine_sim3_candidates(KF1.handle(), &p1, T1w, &v, invLevelSigma2.data(), flat.data(), (int)flat.size(), th,
                                               ORBmatcher::TH_HIGH, th2, bFixScale ? 1 : 0, nfound.data(), results.data());
    if (rc != ORBX_OK) return rc;
    for (size_t k = 0; k < attempts.size(); ++k) {
        RefineSim3Attempt &a = attempts[k];
        a.found12.resize(N1); a.matches12.resize(N1);
        a.nFound = nfound[k]; a.result = results[k];
        if (accepted && *accepted < 0 && a.result.nin >= minInliers) *accepted = (int)k;
    }
    return ORBX_OK;
}

// Initializer (include/Initializer.h, src/Initializer.cc) over orbm_init_find_models / orbm_init_reconstruct_f.  The constructor takes
// what the reference's takes of the reference frame -- mvKeysUn[i].pt of every keypoint, K (3 x 3 row-major), sigma and the iteration
// count -- and Initialize what it takes of the current frame plus a source of draws: a callback int(int lo, int hi) (inclusive, as
// DUtils::Random::RandomInt after SeedRandOnce(0)), called in the reference's order (:82-97), or pre-drawn sets [iterations][8].
// FindHomography and FindFundamental are one launch, ReconstructF's four CheckRT calls one more.
// Two differences to the reference.  ReconstructH (:572-732) is not built: this fork takes it only at RH > 0.99 (:115), and
// Initialize then returns WANTS_RECONSTRUCT_H with H21() and inliersH() for the caller's own ReconstructH.  When no F hypothesis
// scores above 0 the reference leaves vbMatchesInliersF empty and F21 an empty cv::Mat, and ReconstructF throws; here that is
// NO_FUNDAMENTAL.
class Initializer {
public:
    enum Status { NOT_INITIALIZED = 0, INITIALIZED = 1, WANTS_RECONSTRUCT_H = 2, NO_FUNDAMENTAL = 3, FAILED = -1 };   // FAILED: status() has the code
    typedef int (*DrawFn)(int lo, int hi);

    Initializer(std::vector<float> keys1, const float *K, float sigma = 1.0f, int iterations = 200)
        : mvKeys1(std::move(keys1)), mSigma(sigma), mMaxIterations(iterations)
    {
        memcpy(mK, K, sizeof(mK));
        memset(&mModels, 0, sizeof(mModels));
        memset(&mRec, 0, sizeof(mRec));
    }

    // keys2 [n2][2]; vMatches12 [n1]: index into keys2 or -1.  R21 [9], t21 [3], vP3D [n1][3], vbTriangulated [n1].
    Status Initialize(const std::vector<float> &keys2, const std::vector<int> &vMatches12, DrawFn draw, float *R21, float *t21,
                      std::vector<float> &vP3D, std::vector<bool> &vbTriangulated)
    {
        return run(keys2, vMatches12, draw, nullptr, R21, t21, vP3D, vbTriangulated);
    }
    Status Initialize(const std::vector<float> &keys2, const std::vector<int> &vMatches12, const std::vector<int32_t> &sets, float *R21,
                      float *t21, std::vector<float> &vP3D, std::vector<bool> &vbTriangulated)
    {
        return run(keys2, vMatches12, nullptr, &sets, R21, t21, vP3D, vbTriangulated);
    }

    int status() const { return mStatus; }                       // the library's code of the last Initialize
    float RH() const { return mRH; }
    const orbm_init_models &models() const { return mModels; }
    const orbm_init_reconstruction &reconstruction() const { return mRec; }
    const float *H21() const { return mModels.H21; }
    const float *F21() const { return mModels.F21; }
    const std::vector<int32_t> &matches12() const { return mvMatches12; }   // mvMatches12, [n][2]
    const std::vector<int32_t> &sets() const { return mvSets; }             // mvSets, [iterations][8]
    std::vector<bool> inliersH() const { return unpack(mMaskH); }
    std::vector<bool> inliersF() const { return unpack(mMaskF); }

private:
    std::vector<bool> unpack(const std::vector<uint64_t> &mask) const
    {
        const size_t n = mvMatches12.size() / 2;
        std::vector<bool> out(n, false);
        for (size_t i = 0; i < n && i / 64 < mask.size(); ++i) out[i] = (mask[i / 64] >> (i % 64)) & 1;
        return out;
    }

    Status run(const std::vector<float> &keys2, const std::vector<int> &vMatches12, DrawFn draw, const std::vector<int32_t> *sets, float *R21,
               float *t21, std::vector<float> &vP3D, std::vector<bool> &vbTriangulated)
    {
        const int n1 = (int)(mvKeys1.size() / 2), n2 = (int)(keys2.size() / 2);
        mvMatches12.clear();
        for (size_t i = 0; i < vMatches12.size(); ++i)
            if (vMatches12[i] >= 0) { mvMatches12.push_back((int32_t)i); mvMatches12.push_back(vMatches12[i]); }
        const int N = (int)(mvMatches12.size() / 2), H = mMaxIterations;
        vP3D.assign((size_t)3 * n1, 0.0f);
        vbTriangulated.assign((size_t)n1, false);
        for (int k = 0; k < 9; ++k) R21[k] = 0.0f;
        for (int k = 0; k < 3; ++k) t21[k] = 0.0f;
        mRH = std::numeric_limits<float>::quiet_NaN();
        if (draw) {                                              // :77-97
            if (N < 8 && H > 0) { mStatus = ORBX_ERR_ARG; return FAILED; }
            mvSets.assign((size_t)8 * H, 0);
            std::vector<int32_t> avail;
            for (int it = 0; it < H; ++it) {
                avail.resize((size_t)N);
                for (int i = 0; i < N; ++i) avail[i] = i;
                for (int j = 0; j < 8; ++j) {
                    const int randi = draw(0, (int)avail.size() - 1);
                    mvSets[8 * it + j] = avail[randi];
                    avail[randi] = avail.back();
                    avail.pop_back();
                }
            }
        } else {
            if ((int)(sets->size() / 8) < H) { mStatus = ORBX_ERR_ARG; return FAILED; }
            mvSets.assign(sets->begin(), sets->begin() + (size_t)8 * H);
        }
        const size_t words = (size_t)(N + 63) / 64;
        mMaskH.assign(words + 1, 0); mMaskF.assign(words + 1, 0);
        mStatus = orbm_init_find_models(mvKeys1.data(), n1, keys2.data(), n2, mvMatches12.data(), N, mvSets.data(), H, mSigma, &mModels,
                                        mMaskH.data(), mMaskF.data(), nullptr, nullptr, nullptr);
        if (mStatus != ORBX_OK) return FAILED;
        mRH = mModels.SH / (mModels.SH + mModels.SF);            // :112
        if (mRH > 0.99) return WANTS_RECONSTRUCT_H;              // :115
        if (mModels.itF < 0) return NO_FUNDAMENTAL;
        const std::vector<bool> in = inliersF();
        std::vector<uint8_t> inl(in.size() + 1, 0), tri((size_t)n1 + 1, 0);
        for (size_t i = 0; i < in.size(); ++i) inl[i] = in[i];
        mStatus = orbm_init_reconstruct_f(mvKeys1.data(), n1, keys2.data(), n2, mvMatches12.data(), N, inl.data(), mModels.F21, mK, mSigma, 0.95f,
                                          60, &mRec, vP3D.data(), tri.data());
        if (mStatus != ORBX_OK) return FAILED;
        if (!mRec.found) return NOT_INITIALIZED;
        for (int i = 0; i < n1; ++i) vbTriangulated[i] = tri[i] != 0;
        memcpy(R21, mRec.R21, sizeof(mRec.R21));
        memcpy(t21, mRec.t21, sizeof(mRec.t21));
        return INITIALIZED;
    }

    std::vector<float> mvKeys1;
    float mK[9], mSigma;
    int mMaxIterations, mStatus = ORBX_OK;
    float mRH = 0.0f;
    std::vector<int32_t> mvMatches12, mvSets;
    std::vector<uint64_t> mMaskH, mMaskF;
    orbm_init_models mModels;
    orbm_init_reconstruction mRec;
};

// The host half of a KeyFrameDatabase query (src/KeyFrameDatabase.cc:76-309), stated ONCE for both forms and for any way of naming a
// keyframe (Key: a slot number in KeyFrameDatabase below, a KeyFrame* in integration/KeyFrameDatabase_hip.cc).  Input: what
// orbm_kfdb_query leaves per slot -- shared-word count, query index of the first shared word, float L1 score.  The callables:
//   keyOf(slot) -> Key                     of a live slot
//   fieldsOf(Key) -> KfdbQueryFields       the three fields of this FORM that persist across queries (loop: mnLoopQuery, mnLoopWords,
//                                          mLoopScore; relocalisation: mnRelocQuery, mnRelocWords, mRelocScore), by reference
//   connected(Key) -> bool                 loop form: the key is connected to the query keyframe (never asked in the other form)
//   neighbours(Key, std::vector<Key> &)    GetBestCovisibilityKeyFrames(10)
// What it restates: keyframes are met in the order (first shared word, slot); one whose query field already holds this id is
// counted on and not listed again; a connected one ends with a word count of 1 and is not listed; the largest count among the
// LISTED ones gives the cut int(max * 0.8f), strict; the survivors' scores are stored, the loop form then drops those below
// minScore; each remaining one collects the stored scores of its neighbours that this id listed (loop form: and that pass the
// cut; relocalisation form: whatever they hold, also a score of an earlier query) and names the best of the group, a tie staying
// with the earlier; groups above 0.75 of the best total (loop form: of at least minScore) are returned once each, in list order.
struct KfdbQueryFields {
    long unsigned &query;
    int &words;
    float &score;
};

template <class Key, class KeyOf, class FieldsOf, class Connected, class Neighbours>
std::vector<Key> KfdbCandidatesFromCounts(bool loopForm, const int32_t *common, const int32_t *first, const float *score, size_t nslots,
                                          long unsigned id, float minScore, KeyOf keyOf, FieldsOf fieldsOf, Connected connected,
                                          Neighbours neighbours)
{
    struct Entry { Key key; float value; };
    // the sharing slots by (first, slot): a counting sort over `first` that takes the slots in ascending order (at 20,000 keyframes
    // nearly every slot shares a word, and a comparison sort of those was most of this function)
    int maxFirst = -1;
    for (size_t s = 0; s < nslots; ++s)
        if (common[s] > 0) maxFirst = std::max(maxFirst, (int)first[s]);
    std::vector<int> start((size_t)maxFirst + 2, 0), order;
    for (size_t s = 0; s < nslots; ++s)
        if (common[s] > 0) ++start[(size_t)first[s] + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    order.resize((size_t)start.back());
    for (size_t s = 0; s < nslots; ++s)
        if (common[s] > 0) order[(size_t)start[first[s]]++] = (int)s;
    std::vector<Entry> listed;
    for (int s : order) {
        const Key k = keyOf(s);
        KfdbQueryFields f = fieldsOf(k);
        if (f.query == id) { f.words += common[s]; continue; }
        if (loopForm && connected(k)) { f.words = 1; continue; }     // reset at every meeting, then incremented
        f.query = id;
        f.words = common[s];
        listed.push_back(Entry{k, score[s]});
    }
    if (listed.empty()) return std::vector<Key>();
    int most = 0;
    for (const Entry &e : listed) most = std::max(most, fieldsOf(e.key).words);
    const int cut = (int)((float)most * 0.8f);
    std::vector<Entry> kept;
    for (const Entry &e : listed) {
        KfdbQueryFields f = fieldsOf(e.key);
        if (!(f.words > cut)) continue;
        f.score = e.value;
        if (!loopForm || e.value >= minScore) kept.push_back(e);
    }
    if (kept.empty()) return std::vector<Key>();
    float bestTotal = loopForm ? minScore : 0.0f;
    std::vector<Entry> groups;
    std::vector<Key> nb;
    for (const Entry &e : kept) {
        float total = e.value, top = e.value;
        Key winner = e.key;
        nb.clear();
        neighbours(e.key, nb);
        for (const Key &n : nb) {
            KfdbQueryFields g = fieldsOf(n);
            if (g.query != id || (loopForm && !(g.words > cut))) continue;
            total += g.score;
            if (g.score > top) { winner = n; top = g.score; }
        }
        groups.push_back(Entry{winner, total});
        if (total > bestTotal) bestTotal = total;
    }
    const float keepAbove = 0.75f * bestTotal;
    std::vector<Key> out;
    for (const Entry &g : groups)
        if (g.value > keepAbove && std::find(out.begin(), out.end(), g.key) == out.end()) out.push_back(g.key);
    return out;
}

// KeyFrameDatabase (include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc:40-309) over the device store of orbm_kfdb_*: a
// keyframe is known by the SLOT add() returns (ascending in the order of add, restarting at 0 after clear()).  Both Detect
// methods are one orbm_kfdb_query followed by KfdbCandidatesFromCounts over the per-slot fields kept here.
// bestCovisibles(slot, out) fills GetBestCovisibilityKeyFrames(10) of a slot as slots (a neighbour that was never added has no slot
// and is left out: no query can have listed it).  mLoopScore / mRelocScore, which the reference leaves uninitialised, start at
// 0.0f.  A query id of 0 lists nobody, as in the reference (the query fields start at 0).
class KeyFrameDatabase {
public:
    typedef DBoW2::BowVector BowVector;
    struct Fields {                     // KeyFrame.h:160-165
        long unsigned mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0.0f;
        long unsigned mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0.0f;
    };

    explicit KeyFrameDatabase(int nwords) { mStatus = orbm_kfdb_create(nwords, &mDb); }
    ~KeyFrameDatabase() { if (mDb) orbm_kfdb_destroy(mDb); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    // -1: the library refused (status())
    int add(const BowVector &bow)
    {
        flatten(bow);
        int32_t slot = -1;
        mStatus = orbm_kfdb_add(mDb, mWords.data(), mValues.data(), (int)mWords.size(), &slot);
        if (mStatus != ORBX_OK) return -1;
        if ((size_t)slot >= mFields.size()) mFields.resize((size_t)slot + 1);
        mFields[slot] = Fields();
        return slot;
    }
    void erase(int slot) { mStatus = orbm_kfdb_erase(mDb, slot); }
    void clear() { mStatus = orbm_kfdb_clear(mDb); mFields.clear(); }

    // LoopClosing::DetectLoop's minScore loop (LoopClosing.cc:126-138) over the live connected slots: one library call.
    // status() != ORBX_OK afterwards: the library refused and the value is not a score.
    float MinScore(const BowVector &bow, const std::vector<int32_t> &slots)
    {
        float minScore = 1;
        mStatus = ORBX_OK;
        if (slots.empty()) return minScore;
        flatten(bow);
        mScore.resize(slots.size());
        mStatus = orbm_kfdb_score(mDb, mWords.data(), mValues.data(), (int)mWords.size(), slots.data(), (int)slots.size(), mScore.data());
        if (mStatus != ORBX_OK) return minScore;
        for (size_t i = 0; i < slots.size(); ++i)
            if (mScore[i] < minScore) minScore = mScore[i];
        return minScore;
    }

    template <class BestCovisibles>
    std::vector<int> DetectLoopCandidates(const BowVector &bow, long unsigned mnId, const std::vector<int> &connectedSlots, float minScore,
                                          BestCovisibles bestCovisibles)
    {
        if (!query(bow)) return std::vector<int>();
        std::vector<char> connected(mFields.size(), 0);
        for (int c : connectedSlots)
            if (c >= 0 && (size_t)c < connected.size()) connected[c] = 1;
        return KfdbCandidatesFromCounts<int>(
            true, mCommon.data(), mFirst.data(), mScore.data(), mFields.size(), mnId, minScore, [](int s) { return s; },
            [this](int s) { Fields &f = mFields[s]; return KfdbQueryFields{f.mnLoopQuery, f.mnLoopWords, f.mLoopScore}; },
            [&connected](int s) { return connected[s] != 0; }, bestCovisibles);
    }

    template <class BestCovisibles>
    std::vector<int> DetectRelocalizationCandidates(const BowVector &bow, long unsigned mnId, BestCovisibles bestCovisibles)
    {
        if (!query(bow)) return std::vector<int>();
        return KfdbCandidatesFromCounts<int>(
            false, mCommon.data(), mFirst.data(), mScore.data(), mFields.size(), mnId, 0.0f, [](int s) { return s; },
            [this](int s) { Fields &f = mFields[s]; return KfdbQueryFields{f.mnRelocQuery, f.mnRelocWords, f.mRelocScore}; },
            [](int) { return false; }, bestCovisibles);
    }

    const Fields &fields(int slot) const { return mFields[slot]; }
    int slots() const { return (int)mFields.size(); }
    orbm_kfdb *handle() const { return mDb; }
    int status() const { return mStatus; }

private:
    void flatten(const BowVector &bow)
    {
        mWords.clear(); mValues.clear();
        for (BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) { mWords.push_back((int32_t)it->first); mValues.push_back(it->second); }
    }
    bool query(const BowVector &bow)
    {
        flatten(bow);
        const size_t n = mFields.size();
        mCommon.assign(n ? n : 1, 0); mFirst.assign(n ? n : 1, -1); mScore.assign(n ? n : 1, 0.0f);
        mStatus = orbm_kfdb_query(mDb, mWords.data(), mValues.data(), (int)mWords.size(), mCommon.data(), mFirst.data(), mScore.data());
        return mStatus == ORBX_OK;
    }

    orbm_kfdb *mDb = nullptr;
    int mStatus = ORBX_OK;
    std::vector<Fields> mFields;
    std::vector<int32_t> mWords, mCommon, mFirst;
    std::vector<double> mValues;
    std::vector<float> mScore;
};

} // namespace orbslam_hip
#endif // ORBSLAM_HIP_HPP
