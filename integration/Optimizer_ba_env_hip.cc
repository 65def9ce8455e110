// Optimizer_ba_env_hip.cc -- Optimizer::BundleAdjustment (src/Optimizer.cc:74-262) over the map of a LONG session on the device: the
// walk of HipBundleAdjustment (Optimizer_ba_hip.cc), flattened for orbm_global_bundle_adjustment_env, which takes up to
// 4,096 keyframes, 1,048,576 points and 4,194,304 edges.  What differs from that file: the keyframes that are not bad are SORTED BY
// mnId before they get their index, because the order of the free keyframes decides the tile envelope of the reduced system --
// Map::GetAllKeyFrames() comes out of a std::set<KeyFrame *>, that is, in pointer order, and LoopClosing hands that vector over.
// Covisibility is local in time, so in mnId order the blocks form a band, and the points re-observed at a loop widen only the rows
// of the later keyframes.  Reference-side code: compiles in the ORB_SLAM2_E tree.
// Optimizer::BundleAdjustment keeps its body and begins
//     if (HipBundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)) return;
//     if (HipBundleAdjustmentEnv(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)) return;
// It returns false beyond the library's limits (more than 4,096 keyframes, ORBX_ERR_UNSUPPORTED for the other sizes or an envelope of
// more than 8,192 live tiles): the caller keeps g2o there.  Nothing is written to a keyframe or a point before the call has
// returned ORBX_OK, so a refusal leaves the map as it found it.  A point that is bad gets no vertex; one without an edge is left out
// by the library (not_included), as in Optimizer_ba_hip.cc.
#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

namespace {

cv::Mat mat_of(const float *v, int rows, int cols)
{
    cv::Mat M(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) M.at<float>(r, c) = v[cols * r + c];
    return M;
}

} // namespace

bool HipBundleAdjustmentEnv(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP, int nIterations, bool *pbStopFlag,
                            const unsigned long nLoopKF, const bool bRobust)
{
    // ---- :96-108: every keyframe that is not bad is a free vertex (mnId == 0: fixed), in ascending mnId
    std::vector<KeyFrame *> vpUsedKFs;
    for (size_t i = 0; i < vpKFs.size(); i++)
        if (!vpKFs[i]->isBad()) vpUsedKFs.push_back(vpKFs[i]);
    if (nIterations > 64) return false;                                         // (the library's range of optimize(n))
    if (vpUsedKFs.size() > 4096) return false;                                  // orbm_global_bundle_adjustment_env's limit; nothing has been touched
    std::sort(vpUsedKFs.begin(), vpUsedKFs.end(), [](const KeyFrame *a, const KeyFrame *b) { return a->mnId < b->mnId; });
    std::vector<float> poses, points, eObs, eInvSigma2, eCamK;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ePoint, eCam;
    std::map<KeyFrame *, int32_t> kfIndex;
    for (size_t i = 0; i < vpUsedKFs.size(); i++) {
        KeyFrame *pKF = vpUsedKFs[i];
        kfIndex[pKF] = (int32_t)i;
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses.push_back(T.at<float>(r, c));
        fixed.push_back(pKF->mnId == 0 ? 1 : 0);
    }
    const unsigned long maxKFid = vpUsedKFs.empty() ? 0 : vpUsedKFs.back()->mnId;
    // ---- :114-209: the points in vpMP order, a point's observations in the observations map's order
    std::vector<MapPoint *> vpUsedMPs;
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        vpUsedMPs.push_back(pMP);
        const cv::Mat X = pMP->GetWorldPos();
        for (int r = 0; r < 3; r++) points.push_back(X.at<float>(r));
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame *pKF = mit->first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;                  // :134
            const std::map<KeyFrame *, int32_t>::const_iterator it = kfIndex.find(pKF);
            if (it == kfIndex.end()) continue;
            const cv::KeyPoint &kpUn = pKF->mvKeysUn[mit->second];
            ePoint.push_back((int32_t)vpUsedMPs.size() - 1);
            eCam.push_back(it->second);
            eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y); eObs.push_back(pKF->mvuRight[mit->second]);   // ur < 0: the monocular edge
            eInvSigma2.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
            eCamK.push_back(pKF->fx); eCamK.push_back(pKF->fy); eCamK.push_back(pKF->cx); eCamK.push_back(pKF->cy); eCamK.push_back(pKF->mbf);
        }
    }
    if (vpUsedMPs.size() > 1048576 || ePoint.size() > 4194304) return false;    // (the library would say so too)
    const int nfree = (int)vpUsedKFs.size();
    orbm_ba_graph g;
    g.nfree = nfree; g.nfixed = 0; g.npoints = (int32_t)vpUsedMPs.size(); g.nedges = (int32_t)ePoint.size();
    g.poses = poses.data(); g.fixed = fixed.data(); g.points = points.data(); g.e_point = ePoint.data(); g.e_cam = eCam.data();
    g.e_obs = eObs.data(); g.e_inv_sigma2 = eInvSigma2.data(); g.e_cam_k = eCamK.data();
    const orbm_ba_options opt = ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust);
    std::vector<float> posesOut(16 * (size_t)nfree + 1), pointsOut(points.size() + 1);
    std::vector<uint8_t> notIncluded(vpUsedMPs.size() + 1, 0);
    orbm_ba_result res;
    res.poses = posesOut.data(); res.points = pointsOut.data(); res.erase = NULL; res.not_included = notIncluded.data(); res.stopped = 0;
    const int rc = orbm_global_bundle_adjustment_env(&g, &opt, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), &res, NULL);
    if (rc == ORBX_ERR_UNSUPPORTED) return false;
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_global_bundle_adjustment_env: ") + orbx_last_error());

    // ---- :217-260
    for (int k = 0; k < nfree; k++) {
        KeyFrame *pKF = vpUsedKFs[k];
        if (nLoopKF == 0) pKF->SetPose(mat_of(&posesOut[16 * k], 4, 4));
        else {
            pKF->mTcwGBA.create(4, 4, CV_32F);
            mat_of(&posesOut[16 * k], 4, 4).copyTo(pKF->mTcwGBA);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (size_t n = 0; n < vpUsedMPs.size(); n++) {
        if (notIncluded[n]) continue;
        MapPoint *pMP = vpUsedMPs[n];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(mat_of(&pointsOut[3 * n], 3, 1));
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA.create(3, 1, CV_32F);
            mat_of(&pointsOut[3 * n], 3, 1).copyTo(pMP->mPosGBA);
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
    return true;
}

} // namespace ORB_SLAM2
