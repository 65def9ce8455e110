// integration/LocalMapping_create_hip.cc -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:243-520) with its loop over the
// neighbour keyframes as ONE library call (orbm_create_new_map_points): the shell keeps the baseline test, ComputeF12 and the
// pointer graph, flattens the keyframes, makes the call and replays the creation list in the reference's order.
//
// Written against the patched headers of reference.patch (KeyFrame::mpHipFrame); like the other shells it cannot be compiled where
// OpenCV / DBoW2 are absent, and reference.patch does not carry it (its hunks are pinned): it replaces the body of
// LocalMapping::CreateNewMapPoints when added to the reference's CMakeLists.txt in place of that definition.
//
// One call cannot be interrupted: the reference's `if(i>0 && CheckNewKeyFrames()) return;` (:283) between neighbours is given up
// inside a call.  kChunk below restores it at a coarser grain: the neighbours go in chunks, with the check between chunks.
#include "LocalMapping.h"
#include "ORBmatcher.h"

#include <iostream>
#include <memory>

#include "orbslam_hip.h"

namespace ORB_SLAM2
{

namespace
{
// DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>) in map order
struct FlatFeatVec {
    std::vector<int32_t> nodes, off, items;
    explicit FlatFeatVec(const DBoW2::FeatureVector &fv)
    {
        off.push_back(0);
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
            nodes.push_back((int32_t)it->first);
            items.insert(items.end(), it->second.begin(), it->second.end());
            off.push_back((int32_t)items.size());
        }
    }
};

// What orbm_create_new_map_points reads of a keyframe; the arrays live as long as this object
struct FlatKeyFrame {
    cv::Mat Tcw;
    FlatFeatVec fv;
    std::vector<uint8_t> has;
    float F12[9];
    orbm_triang_keyframe c;
    explicit FlatKeyFrame(KeyFrame *pKF) : Tcw(pKF->GetPose().clone()), fv(pKF->mFeatVec), has(pKF->N, 0)
    {
        for (int i = 0; i < pKF->N; ++i) has[i] = pKF->GetMapPoint(i) != NULL;
        c.frame = pKF->mpHipFrame.get();
        c.Tcw = Tcw.ptr<float>(0);
        c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy; c.invfx = pKF->invfx; c.invfy = pKF->invfy;
        c.mb = pKF->mb; c.mbf = pKF->mbf;
        c.depth = pKF->mvDepth.empty() ? NULL : pKF->mvDepth.data();
        c.has_mappoint = has.data();
        c.nodes = fv.nodes.data(); c.off = fv.off.data(); c.items = fv.items.data(); c.nn = (int32_t)fv.nodes.size();
        c.F12 = NULL; c.ex = 0.f; c.ey = 0.f;
    }
};
const int kChunk = 32;     // neighbours per call (at most 32); smaller: CheckNewKeyFrames() is looked at more often
}

void LocalMapping::CreateNewMapPoints()
{
    nBaselineRejects = 0; nTriangulationRejects = 0; nParalaxRejects = 0; nRepErrorRejects = 0; nScaleConsRejects = 0; nDepthRejects = 0;
    int nn = 10;
    if (mbMonocular) nn = 20;
    const vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    cv::Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();

    // the neighbours that pass the baseline test (:288-308), in order: stereo / RGB-D wants a baseline of at least the rig's own,
    // monocular one of at least 5 % of the neighbour's median scene depth (and counts the others)
    vector<KeyFrame*> vpUsed;
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        KeyFrame *pKF2 = vpNeighKFs[i];
        const float baseline = cv::norm(pKF2->GetCameraCenter() - Ow1);
        bool use;
        if (mbMonocular) {
            use = !(baseline / pKF2->ComputeSceneMedianDepth(2) < 0.05);
            if (!use) nBaselineRejects++;
        } else
            use = !(baseline < pKF2->mb);
        if (use) vpUsed.push_back(pKF2);
    }

    for (size_t first = 0; first < vpUsed.size(); first += kChunk) {
        if (first > 0 && CheckNewKeyFrames()) return;                                    // :283, between chunks
        const int K = (int)std::min(vpUsed.size() - first, (size_t)kChunk);
        FlatKeyFrame cur(mpCurrentKeyFrame);         // (again per chunk: the mask holds the points of the chunks before)
        vector<std::unique_ptr<FlatKeyFrame> > flat;
        vector<orbm_triang_keyframe> neigh;
        for (int k = 0; k < K; ++k) {
            KeyFrame *pKF2 = vpUsed[first + k];
            std::unique_ptr<FlatKeyFrame> f(new FlatKeyFrame(pKF2));
            cv::Mat F12 = ComputeF12(mpCurrentKeyFrame, pKF2);                          // :311
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) f->F12[3 * r + c] = F12.at<float>(r, c);
            cv::Mat C2 = pKF2->GetRotation() * Ow1 + pKF2->GetTranslation();            // the epipole, ORBmatcher.cc:863-871
            const float invz = 1.0f / C2.at<float>(2);
            f->c.F12 = f->F12;
            f->c.ex = pKF2->fx * C2.at<float>(0) * invz + pKF2->cx;
            f->c.ey = pKF2->fy * C2.at<float>(1) * invz + pKF2->cy;
            neigh.push_back(f->c);
            flat.push_back(std::move(f));
        }
        const int n1 = mpCurrentKeyFrame->N;
        const size_t kn = (size_t)K * (size_t)n1;
        vector<int32_t> match12(kn ? kn : 1), counts((size_t)K * ORBM_TRI_NSTATUS);
        vector<int8_t> status(kn ? kn : 1);
        vector<float> x3d(3 * (kn ? kn : 1));
        int nnew = 0;
        const int rc = orbm_create_new_map_points(&cur.c, neigh.data(), K, mpCurrentKeyFrame->mvScaleFactors.data(),
                                                  mpCurrentKeyFrame->mvLevelSigma2.data(), mpCurrentKeyFrame->mnScaleLevels,
                                                  mpCurrentKeyFrame->mfScaleFactor, match12.data(), status.data(), x3d.data(), counts.data(),
                                                  &nnew);
        if (rc != ORBX_OK) {       // nothing of this chunk is applied; what earlier chunks created stays, as after the reference's early return
            std::cerr << "CreateNewMapPoints: orbm_create_new_map_points failed (" << rc << "): " << orbx_last_error() << std::endl;
            bDataToSave = true;
            return;
        }
        // :499-515 over the creation list, (k, idx1) ascending: the reference's order
        for (int k = 0; k < K; ++k) {
            KeyFrame *pKF2 = vpUsed[first + k];
            const int32_t *ck = counts.data() + (size_t)k * ORBM_TRI_NSTATUS;
            nTriangulationRejects += ck[ORBM_TRI_SVD_ZERO]; nParalaxRejects += ck[ORBM_TRI_PARALLAX]; nDepthRejects += ck[ORBM_TRI_DEPTH];
            nRepErrorRejects += ck[ORBM_TRI_REPROJ1]; nScaleConsRejects += ck[ORBM_TRI_SCALE];
            for (int i = 0; i < n1; ++i) {
                const size_t o = (size_t)k * n1 + i;
                if (status[o] != ORBM_TRI_CREATED) continue;
                const int idx2 = match12[o];
                cv::Mat x3D = (cv::Mat_<float>(3, 1) << x3d[3 * o], x3d[3 * o + 1], x3d[3 * o + 2]);
                MapPoint *pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);
                pMP->AddObservation(mpCurrentKeyFrame, i); pMP->AddObservation(pKF2, idx2);
                mpCurrentKeyFrame->AddMapPoint(pMP, i); pKF2->AddMapPoint(pMP, idx2);
                pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth();
                mpMap->AddMapPoint(pMP); mlpRecentAddedMapPoints.push_back(pMP);
            }
        }
    }
    bDataToSave = true;
}

} // namespace ORB_SLAM2
