// Optimizer_essential_graph_env_hip.cc -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1165-1428) of a LONG session on the device:
// the walk of Optimizer_essential_graph_hip.cc, flattened for orbm_essential_graph_env, which takes up to 4,096 free
// keyframes with an edge, 8,192 keyframes, 131,072 edges and 1,048,576 points.  What differs from that file: the keyframes that are
// not bad are SORTED BY mnId before they get their vertex index, because the order of the vertices decides the tile envelope of the
// system (spanning-tree and covisibility edges then join neighbours in the list); the edges are still created in the reference's
// order, by the same walk over GetAllKeyFrames().  Reference-side code: compiles in the ORB_SLAM2_E tree.
// the function keeps its body and begins
//     if (HipOptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)) return;
//     if (HipOptimizeEssentialGraphEnv(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)) return;
// It returns false beyond the library's limits (ORBX_ERR_UNSUPPORTED: the sizes above, or an envelope of more than 8,192 live
// tiles): the caller keeps g2o there.  Nothing is written before the call returns ORBX_OK, so a refusal leaves the map as it found it.
// Edges and points that have no vertex are treated as in Optimizer_essential_graph_hip.cc.
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapPoint.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2 {

namespace {

// the CorrectedSim3 / NonCorrectedSim3 entry of pKF as a row of the table (q xyzw, t, s), or -1
int32_t table_row(const LoopClosing::KeyFrameAndPose &table, KeyFrame *pKF, std::vector<double> &rows)
{
    const LoopClosing::KeyFrameAndPose::const_iterator it = table.find(pKF);
    if (it == table.end()) return -1;
    const g2o::Sim3 &S = it->second;
    for (int k = 0; k < 4; k++) rows.push_back(S.rotation().coeffs()[k]);
    for (int k = 0; k < 3; k++) rows.push_back(S.translation()[k]);
    rows.push_back(S.scale());
    return (int32_t)(rows.size() / 8) - 1;
}

} // namespace

bool HipOptimizeEssentialGraphEnv(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                  const LoopClosing::KeyFrameAndPose &CorrectedSim3, const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections,
                                  const bool &bFixScale)
{
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const int minFeat = 100;

    // ---- :1193-1228: a vertex per keyframe that is not bad, in ascending mnId
    std::vector<float> poses, points;
    std::vector<int32_t> corrected, noncorrected, eV0, eV1, pRef;
    std::vector<double> correctedSim3, noncorrectedSim3;
    std::vector<uint8_t> fixed, eKind;
    std::vector<KeyFrame *> vpUsedKFs;
    std::map<KeyFrame *, int32_t> kfIndex;
    std::map<long unsigned int, int32_t> idIndex;
    for (size_t i = 0; i < vpKFs.size(); i++)
        if (!vpKFs[i]->isBad()) vpUsedKFs.push_back(vpKFs[i]);
    if (vpUsedKFs.size() > 8192) return false;                                 // the library's limit; nothing has been touched
    std::sort(vpUsedKFs.begin(), vpUsedKFs.end(), [](const KeyFrame *a, const KeyFrame *b) { return a->mnId < b->mnId; });
    for (size_t i = 0; i < vpUsedKFs.size(); i++) {
        KeyFrame *pKF = vpUsedKFs[i];
        kfIndex[pKF] = idIndex[pKF->mnId] = (int32_t)i;
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses.push_back(T.at<float>(r, c));
        corrected.push_back(table_row(CorrectedSim3, pKF, correctedSim3));
        noncorrected.push_back(table_row(NonCorrectedSim3, pKF, noncorrectedSim3));
        fixed.push_back(pKF == pLoopKF ? 1 : 0);
    }
    struct Edges {
        const std::map<KeyFrame *, int32_t> &index;
        std::vector<int32_t> &v0, &v1;
        std::vector<uint8_t> &kind;
        void add(KeyFrame *pKFi, KeyFrame *pKFj, int k)
        {
            const std::map<KeyFrame *, int32_t>::const_iterator a = index.find(pKFi), b = index.find(pKFj);
            if (a == index.end() || b == index.end() || a->second == b->second) return;
            v0.push_back(a->second); v1.push_back(b->second); kind.push_back((uint8_t)k);
        }
    } edges = {kfIndex, eV0, eV1, eKind};

    // ---- :1236-1264: the LoopConnections edges, measured between the vScw of both sides
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame *> &spConnections = mit->second;
        for (std::set<KeyFrame *>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            edges.add(pKF, *sit, 0);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // ---- :1267-1367: the spanning tree, the old loop edges and the covisibility edges, each side through its NonCorrectedSim3
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        KeyFrame *pParentKF = pKF->GetParent();
        if (pParentKF) edges.add(pKF, pParentKF, 1);
        const std::set<KeyFrame *> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<KeyFrame *>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++)
            if ((*sit)->mnId < pKF->mnId) edges.add(pKF, *sit, 1);
        const std::vector<KeyFrame *> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<KeyFrame *>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    edges.add(pKF, pKFn, 1);
                }
            }
        }
    }
    // ---- :1397-1413: the points and the keyframe each is corrected through
    std::vector<MapPoint *> vpUsedMPs, vpOtherMPs;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const std::map<long unsigned int, int32_t>::const_iterator it = idIndex.find(nIDr);
        if (it == idIndex.end()) { vpOtherMPs.push_back(pMP); continue; }
        const cv::Mat X = pMP->GetWorldPos();
        for (int r = 0; r < 3; r++) points.push_back(X.at<float>(r));
        pRef.push_back(it->second);
        vpUsedMPs.push_back(pMP);
    }

    orbm_eg_graph g;
    g.nvert = (int32_t)vpUsedKFs.size(); g.ncorr = (int32_t)(correctedSim3.size() / 8); g.nnc = (int32_t)(noncorrectedSim3.size() / 8);
    g.nedges = (int32_t)eV0.size(); g.npoints = (int32_t)vpUsedMPs.size(); g.fix_scale = bFixScale ? 1 : 0;
    g.poses = poses.data(); g.corrected = corrected.data(); g.corrected_sim3 = correctedSim3.data();
    g.noncorrected = noncorrected.data(); g.noncorrected_sim3 = noncorrectedSim3.data(); g.fixed = fixed.data();
    g.e_v0 = eV0.data(); g.e_v1 = eV1.data(); g.e_kind = eKind.data(); g.points = points.data(); g.p_ref = pRef.data();
    const orbm_eg_options opt = ORBM_EG_OPTIONS_DEFAULT;                        // optimize(20), setUserLambdaInit(1e-16)
    std::vector<float> posesOut(poses.size() + 1), pointsOut(points.size() + 1);
    orbm_eg_result res;
    res.poses = posesOut.data(); res.points = pointsOut.data();
    const int rc = orbm_essential_graph_env(&g, &opt, &res, NULL);
    if (rc == ORBX_ERR_UNSUPPORTED) return false;
    if (rc != ORBX_OK) throw std::runtime_error(std::string("orbm_essential_graph_env: ") + orbx_last_error());

    // ---- :1373-1427
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (size_t k = 0; k < vpUsedKFs.size(); k++) {
        cv::Mat Tiw(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tiw.at<float>(r, c) = posesOut[16 * k + 4 * r + c];
        vpUsedKFs[k]->SetPose(Tiw);
    }
    for (size_t n = 0; n < vpUsedMPs.size(); n++) {
        cv::Mat X(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) X.at<float>(r) = pointsOut[3 * n + r];
        vpUsedMPs[n]->SetWorldPos(X);
        vpUsedMPs[n]->UpdateNormalAndDepth();
    }
    for (size_t n = 0; n < vpOtherMPs.size(); n++) vpOtherMPs[n]->UpdateNormalAndDepth();
    return true;
}

} // namespace ORB_SLAM2
