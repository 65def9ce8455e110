// Optimizer_ba_hip.cc -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:837-1162) and Optimizer::BundleAdjustment (:74-262) with
// the optimisation on the device.  The walks over KeyFrame* / MapPoint* (:839-1037, :96-209) stay here, on the host, and fill the flat
// graph of orbm_bundle_adjustment instead of a g2o::SparseOptimizer; both rounds of optimize(), the level pass between them and the
// final pass (:1043-1127), or the one optimize(nIterations) (:211-213), are ONE library call; the erase loop and the write-back
// (:1130-1161, :217-260 with mTcwGBA / mPosGBA) are the reference's, here.  Reference-side code: compiles in the ORB_SLAM2_E tree.
// the two functions keep their bodies and gain one first line each,
//     if (HipLocalBundleAdjustment(pKF, pbStopFlag, pMap)) return;
//     if (HipBundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)) return;
// Both return false beyond the library's limits (ORBX_ERR_UNSUPPORTED: more than 64 local keyframes, 1,024 fixed ones, 65,536
// points or 524,288 edges; for BundleAdjustment more than 512 keyframes -- the global BA after a loop closure of a long session):
// the caller keeps g2o there.  BundleAdjustment over more than 64 keyframes (LoopClosing::RunGlobalBundleAdjustment's
// GlobalBundleAdjustemnt over the whole map) goes through orbm_global_bundle_adjustment, whose reduced system is solved by the tiled
// multi-workgroup Cholesky; up to 64 it keeps orbm_bundle_adjustment.  A refusal leaves
// the map as it found it: BundleAdjustment's walk writes nothing, and LocalBundleAdjustment's walk, which marks keyframes and points
// with mnBALocalForKF / mnBAFixedForKF and tests those marks, counts the local keyframes before it marks anything and puts every
// mark back when a later limit refuses, so that the reference's walk behind it finds what it would have found without the shell.
// One thing of :1043-1127 is NOT reproduced: `if (pMP->isBad()) continue;` (:1061, :1104) inside the two passes.  They run inside the
// call on the graph as it was flattened, so a map point another thread marks bad WHILE the call runs is classified like the others;
// the erase loop below skips it instead (EraseMapPointMatch / EraseObservation of a bad point are no-ops in the reference).
#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

namespace {

void push_pose(std::vector<float> &dst, const cv::Mat &T)       // 4 x 4 CV_32F, row-major
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) dst.push_back(T.at<float>(r, c));
}

struct FlatGraph {
    std::vector<float> poses, points, eObs, eInvSigma2, eCamK;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ePoint, eCam;
    std::vector<KeyFrame *> edgeKF;
    std::vector<MapPoint *> edgeMP;

    void addPoint(MapPoint *pMP)
    {
        const cv::Mat X = pMP->GetWorldPos();
        for (int r = 0; r < 3; r++) points.push_back(X.at<float>(r));
    }
    // an observation of the last added point: :975-1034 / :139-197
    void addEdge(MapPoint *pMP, KeyFrame *pKFi, size_t idx, int32_t cam)
    {
        const cv::KeyPoint &kpUn = pKFi->mvKeysUn[idx];
        ePoint.push_back((int32_t)(points.size() / 3) - 1);
        eCam.push_back(cam);
        eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y); eObs.push_back(pKFi->mvuRight[idx]);      // ur < 0: the monocular edge
        eInvSigma2.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
        eCamK.push_back(pKFi->fx); eCamK.push_back(pKFi->fy); eCamK.push_back(pKFi->cx); eCamK.push_back(pKFi->cy); eCamK.push_back(pKFi->mbf);
        edgeKF.push_back(pKFi); edgeMP.push_back(pMP);
    }
    orbm_ba_graph c(int nfree) const
    {
        orbm_ba_graph g;
        g.nfree = nfree; g.nfixed = (int32_t)(poses.size() / 16) - nfree; g.npoints = (int32_t)(points.size() / 3); g.nedges = (int32_t)ePoint.size();
        g.poses = poses.data(); g.fixed = fixed.data(); g.points = points.data(); g.e_point = ePoint.data(); g.e_cam = eCam.data();
        g.e_obs = eObs.data(); g.e_inv_sigma2 = eInvSigma2.data(); g.e_cam_k = eCamK.data();
        return g;
    }
};

cv::Mat pose_mat(const float *T)
{
    cv::Mat M(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) M.at<float>(r, c) = T[4 * r + c];
    return M;
}
cv::Mat point_mat(const float *X)
{
    cv::Mat M(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) M.at<float>(r) = X[r];
    return M;
}

} // namespace

bool HipLocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap)
{
    // ---- :839-888.  The walk marks keyframes and map points (mnBALocalForKF, mnBAFixedForKF) and tests those marks itself, so a
    // refusal must not leave them behind: the reference's body, which then runs, would find every point marked already (:864) and
    // build an empty graph.  The number of local keyframes is checked before anything is marked, and every mark is recorded with
    // the value it replaces and put back if the library refuses.
    const std::vector<KeyFrame *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    {
        size_t nLocal = 1;
        for (size_t i = 0; i < vNeighKFs.size(); i++) nLocal += !vNeighKFs[i]->isBad();
        if (nLocal > 64) return false;                                          // the library's limit; nothing has been touched
    }
    std::vector<std::pair<long unsigned int *, long unsigned int> > marks;      // (the member, its value before)
    struct Mark {
        static void set(std::vector<std::pair<long unsigned int *, long unsigned int> > &m, long unsigned int &member, long unsigned int v)
        {
            m.push_back(std::make_pair(&member, member));
            member = v;
        }
        static void undo(std::vector<std::pair<long unsigned int *, long unsigned int> > &m)
        {
            for (size_t i = m.size(); i-- > 0;) *m[i].first = m[i].second;
        }
    };
    std::list<KeyFrame *> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    Mark::set(marks, pKF->mnBALocalForKF, pKF->mnId);
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame *pKFi = vNeighKFs[i];
        Mark::set(marks, pKFi->mnBALocalForKF, pKF->mnId);
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    std::list<MapPoint *> lLocalMapPoints;
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        std::vector<MapPoint *> vpMPs = (*lit)->GetMapPointMatches();
        for (std::vector<MapPoint *>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint *pMP = *vit;
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                Mark::set(marks, pMP->mnBALocalForKF, pKF->mnId);
            }
        }
    }
    std::list<KeyFrame *> lFixedCameras;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        std::map<KeyFrame *, size_t> observations = (*lit)->GetObservations();
        for (std::map<KeyFrame *, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                Mark::set(marks, pKFi->mnBAFixedForKF, pKF->mnId);
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }
    // ---- :907-1037 into the flat graph: the local keyframes first (mnId == 0: fixed, :913), then the fixed ones
    FlatGraph G;
    std::map<KeyFrame *, int32_t> kfIndex;
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        kfIndex[*lit] = (int32_t)(G.poses.size() / 16);
        push_pose(G.poses, (*lit)->GetPose());
        G.fixed.push_back((*lit)->mnId == 0 ? 1 : 0);
    }
    const int nfree = (int)lLocalKeyFrames.size();
    for (std::list<KeyFrame *>::iterator lit = lFixedCameras.begin(), lend = lFixedCameras.end(); lit != lend; lit++) {
        kfIndex[*lit] = (int32_t)(G.poses.size() / 16);
        push_pose(G.poses, (*lit)->GetPose());
    }
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        MapPoint *pMP = *lit;
        G.addPoint(pMP);
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->isBad()) continue;                                        // :973
            const std::map<KeyFrame *, int32_t>::const_iterator it = kfIndex.find(pKFi);
            if (it == kfIndex.end()) continue;                                  // (a bad keyframe that was not listed: optimizer.vertex() is NULL there)
            G.addEdge(pMP, pKFi, mit->second, it->second);
        }
    }
    // ---- :1039-1127: the stop flag before the first optimize, optimize(5), the level pass, optimize(10), the final pass
    const orbm_ba_graph g = G.c(nfree);
    const orbm_ba_options opt = ORBM_BA_OPTIONS_LOCAL;
    std::vector<float> posesOut(16 * (size_t)nfree + 1), pointsOut(G.points.size() + 1);
    std::vector<uint8_t> erase(G.ePoint.size() + 1, 0);
    orbm_ba_result res;
    res.poses = posesOut.data(); res.points = pointsOut.data(); res.erase = erase.data(); res.not_included = NULL; res.stopped = 0;
    const int rc = orbm_bundle_adjustment(&g, &opt, reinterpret_cast<const volatile uint8_t *>(pbStopFlag), &res, NULL);
    if (rc == ORBX_ERR_UNSUPPORTED) {                                           // a later limit (fixed keyframes, points, edges)
        Mark::undo(marks);                                                      // the reference's walk starts from the marks it would have found
        return false;
    }
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_bundle_adjustment: ") + orbx_last_error());
    if (res.stopped == 1) return true;                                          // :1039-1041: return with nothing changed

    // ---- :1129-1161
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (size_t e = 0; e < G.ePoint.size(); e++) {
        if (!erase[e] || G.edgeMP[e]->isBad()) continue;                        // :1104
        G.edgeKF[e]->EraseMapPointMatch(G.edgeMP[e]);
        G.edgeMP[e]->EraseObservation(G.edgeKF[e]);
    }
    int k = 0;
    for (std::list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++, k++)
        (*lit)->SetPose(pose_mat(&posesOut[16 * k]));
    int n = 0;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++, n++) {
        (*lit)->SetWorldPos(point_mat(&pointsOut[3 * n]));
        (*lit)->UpdateNormalAndDepth();
    }
    return true;
}

bool HipBundleAdjustment(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP, int nIterations, bool *pbStopFlag,
                         const unsigned long nLoopKF, const bool bRobust)
{
    // ---- :96-108: every keyframe that is not bad is a free vertex (mnId == 0: fixed); there are no other keyframes
    FlatGraph G;
    std::map<KeyFrame *, int32_t> kfIndex;
    std::vector<KeyFrame *> vpUsedKFs;
    unsigned long maxKFid = 0;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        kfIndex[pKF] = (int32_t)vpUsedKFs.size();
        vpUsedKFs.push_back(pKF);
        push_pose(G.poses, pKF->GetPose());
        G.fixed.push_back(pKF->mnId == 0 ? 1 : 0);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }
    if (nIterations > 64) return false;                                         // (the library's range of optimize(n))
    if (vpUsedKFs.size() > 512) return false;                                   // orbm_global_bundle_adjustment's limit; nothing has been touched
    // ---- :114-209: a point that is bad gets no vertex; one without an edge is left out by the library (not_included)
    std::vector<MapPoint *> vpUsedMPs;
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        vpUsedMPs.push_back(pMP);
        G.addPoint(pMP);
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame *pKF = mit->first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;                  // :134
            const std::map<KeyFrame *, int32_t>::const_iterator it = kfIndex.find(pKF);
            if (it == kfIndex.end()) continue;
            G.addEdge(pMP, pKF, mit->second, it->second);
        }
    }
    const int nfree = (int)vpUsedKFs.size();
    const orbm_ba_graph g = G.c(nfree);
    const orbm_ba_options opt = ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust);
    std::vector<float> posesOut(16 * (size_t)nfree + 1), pointsOut(G.points.size() + 1);
    std::vector<uint8_t> notIncluded(vpUsedMPs.size() + 1, 0);
    orbm_ba_result res;
    res.poses = posesOut.data(); res.points = pointsOut.data(); res.erase = NULL; res.not_included = notIncluded.data(); res.stopped = 0;
    const volatile uint8_t *stop = reinterpret_cast<const volatile uint8_t *>(pbStopFlag);
    const int rc = nfree > 64 ? orbm_global_bundle_adjustment(&g, &opt, stop, &res, NULL) : orbm_bundle_adjustment(&g, &opt, stop, &res, NULL);
    if (rc == ORBX_ERR_UNSUPPORTED) return false;
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_bundle_adjustment: ") + orbx_last_error());

    // ---- :217-260
    for (int k = 0; k < nfree; k++) {
        KeyFrame *pKF = vpUsedKFs[k];
        if (nLoopKF == 0) pKF->SetPose(pose_mat(&posesOut[16 * k]));
        else {
            pKF->mTcwGBA.create(4, 4, CV_32F);
            pose_mat(&posesOut[16 * k]).copyTo(pKF->mTcwGBA);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (size_t n = 0; n < vpUsedMPs.size(); n++) {
        if (notIncluded[n]) continue;
        MapPoint *pMP = vpUsedMPs[n];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(point_mat(&pointsOut[3 * n]));
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA.create(3, 1, CV_32F);
            point_mat(&pointsOut[3 * n]).copyTo(pMP->mPosGBA);
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
    return true;
}

} // namespace ORB_SLAM2
