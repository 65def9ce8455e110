// integration/ORBmatcher_bow_batch_hip.cc -- the two loops that call ORBmatcher::SearchByBoW once per candidate keyframe, each as
// ONE library call (orbm_frame_search_by_bow_pairs):
//   HipSearchByBoWCandidates      Tracking::Relocalization     src/Tracking.cc:1768-1795      SearchByBoW(pKF, mCurrentFrame, ...)
//   HipSearchByBoWLoopCandidates  LoopClosing::ComputeSim3     src/LoopClosing.cc:252-280     SearchByBoW(mpCurrentKF, pKF, ...)
// The shells keep the pointer graph -- isBad(), GetMapPointMatches(), the write-back into the MapPoint* vectors -- and flatten
// every mFeatVec once; the frame all pairs share (the current frame / the current keyframe) is flattened once, not once per pair.
//
// Written against the patched headers of reference.patch (Frame::mpHipFrame / KeyFrame::mpHipFrame); like the other shells it
// cannot be compiled where OpenCV / DBoW2 are absent, and reference.patch does not carry it (its hunks are pinned).  The callers'
// loops are replaced by hand, see INTEGRATION.md section 2: vnMatches[i] is the nmatches of the reference's iteration i, and
// -1 where the reference skips the candidate (isBad()); everything behind the SearchByBoW call of an iteration stays as it is.
#include <algorithm>
#include <memory>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "hip_frame.h"
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

// What a pair reads of a keyframe: its resident frame, its flat mFeatVec, "owns a good MapPoint" per keypoint (ORBmatcher.cc:395-399,
// :763-767, :782-786) and the points themselves for the write-back.  The arrays live as long as this object.
struct FlatKeyFrame {
    const orbm_frame *frame;
    int N;
    FlatFeatVec fv;
    std::vector<MapPoint*> vpMapPoints;
    std::vector<uint8_t> valid;
    std::vector<int32_t> match12;
    explicit FlatKeyFrame(KeyFrame *pKF)
        : frame(pKF->mpHipFrame.get()), N(pKF->N), fv(pKF->mFeatVec), vpMapPoints(pKF->GetMapPointMatches()), valid(pKF->N > 0 ? pKF->N : 1, 0)
    {
        for (int i = 0; i < N; ++i) valid[i] = vpMapPoints[i] && !vpMapPoints[i]->isBad();
    }
    void first_of(orbm_bow_pair &p) const
    {
        p.frame1 = frame; p.nodes1 = fv.nodes.data(); p.off1 = fv.off.data(); p.items1 = fv.items.data(); p.nn1 = (int32_t)fv.nodes.size();
        p.valid1 = valid.data();
    }
    void second_of(orbm_bow_pair &p) const
    {
        p.frame2 = frame; p.nodes2 = fv.nodes.data(); p.off2 = fv.off.data(); p.items2 = fv.items.data(); p.nn2 = (int32_t)fv.nodes.size();
        p.valid2 = valid.data();
    }
};

const size_t kMaxPairs = 64;      // pairs per library call; longer candidate lists go in chunks

// the library call over pairs [0, K) in chunks of kMaxPairs: false if a chunk failed
bool SearchPairs(const std::vector<orbm_bow_pair> &pairs, int strict_th, float nnratio, bool checkOri, std::vector<int32_t> &nm)
{
    nm.assign(pairs.size() ? pairs.size() : 1, 0);
    for (size_t k0 = 0; k0 < pairs.size(); k0 += kMaxPairs) {
        const size_t K = std::min(kMaxPairs, pairs.size() - k0);
        if (orbm_frame_search_by_bow_pairs(&pairs[k0], (int)K, ORBmatcher::TH_LOW, strict_th, nnratio, checkOri ? 1 : 0, &nm[k0]) != ORBX_OK)
            return false;
    }
    return true;
}
}

// Tracking::Relocalization's first stage (src/Tracking.cc:1768-1795).  vvpMapPointMatches[i] and vnMatches[i] are what
// matcher.SearchByBoW(vpCandidateKFs[i], F, vvpMapPointMatches[i]) gives (nnratio / checkOri: the matcher's; 0.75 / true at both call sites);
// vnMatches[i] = -1 and vvpMapPointMatches[i] untouched where the candidate isBad() (the reference sets vbDiscarded[i] and goes on).
// Returns false if the library refused the call (nothing is written then).
bool HipSearchByBoWCandidates(const std::vector<KeyFrame*> &vpCandidateKFs, Frame &F, std::vector<std::vector<MapPoint*> > &vvpMapPointMatches,
                              std::vector<int> &vnMatches, float nnratio = 0.75f, bool checkOri = true)
{
    const size_t nKFs = vpCandidateKFs.size();
    const FlatFeatVec fvF(F.mFeatVec);              // the current frame: second of every pair, flattened once
    std::vector<std::unique_ptr<FlatKeyFrame> > kfs;
    std::vector<size_t> which;
    std::vector<orbm_bow_pair> pairs;
    for (size_t i = 0; i < nKFs; ++i) {
        if (vpCandidateKFs[i]->isBad()) continue;   // :1771-1772
        kfs.push_back(std::unique_ptr<FlatKeyFrame>(new FlatKeyFrame(vpCandidateKFs[i])));
        FlatKeyFrame &kf = *kfs.back();
        kf.match12.assign(kf.N > 0 ? kf.N : 1, -1);
        orbm_bow_pair p;
        kf.first_of(p);
        p.frame2 = F.mpHipFrame.get(); p.nodes2 = fvF.nodes.data(); p.off2 = fvF.off.data(); p.items2 = fvF.items.data();
        p.nn2 = (int32_t)fvF.nodes.size(); p.valid2 = NULL;                     // the Frame form: every feature of F is a candidate
        p.match12 = kf.match12.data(); p.match21 = NULL;
        pairs.push_back(p); which.push_back(i);
    }
    std::vector<int32_t> nm;
    if (!SearchPairs(pairs, /*strict_th=*/0, nnratio, checkOri, nm)) return false;
    vnMatches.assign(nKFs, -1);
    vvpMapPointMatches.resize(nKFs);
    for (size_t k = 0; k < pairs.size(); ++k) {
        const FlatKeyFrame &kf = *kfs[k];
        std::vector<MapPoint*> &vpMapPointMatches = vvpMapPointMatches[which[k]];
        vpMapPointMatches = std::vector<MapPoint*>(F.N, static_cast<MapPoint*>(NULL));
        for (int i = 0; i < kf.N; ++i)
            if (kf.match12[i] >= 0) vpMapPointMatches[kf.match12[i]] = kf.vpMapPoints[i];              // ORBmatcher.cc:433
        vnMatches[which[k]] = nm[k];
    }
    return true;
}

// LoopClosing::ComputeSim3's first stage (src/LoopClosing.cc:252-280).  vvpMapPointMatches[i] and vnMatches[i] are what
// matcher.SearchByBoW(pCurrentKF, vpCandidates[i], vvpMapPointMatches[i]) gives; -1 / untouched where the candidate isBad().
// SetNotErase() on every candidate (:257) stays with the caller, in front of this call.
bool HipSearchByBoWLoopCandidates(KeyFrame *pCurrentKF, const std::vector<KeyFrame*> &vpCandidates,
                                  std::vector<std::vector<MapPoint*> > &vvpMapPointMatches, std::vector<int> &vnMatches,
                                  float nnratio = 0.75f, bool checkOri = true)
{
    const size_t nKFs = vpCandidates.size();
    const FlatKeyFrame cur(pCurrentKF);             // the current keyframe: first of every pair, flattened once
    std::vector<std::unique_ptr<FlatKeyFrame> > kfs;
    std::vector<size_t> which;
    std::vector<orbm_bow_pair> pairs;
    for (size_t i = 0; i < nKFs; ++i) {
        if (vpCandidates[i]->isBad()) continue;     // :259-263
        kfs.push_back(std::unique_ptr<FlatKeyFrame>(new FlatKeyFrame(vpCandidates[i])));
        FlatKeyFrame &kf = *kfs.back();
        kf.match12.assign(cur.N > 0 ? cur.N : 1, -1);           // (the pair's row runs over the CURRENT keyframe's keypoints)
        orbm_bow_pair p;
        cur.first_of(p);
        kf.second_of(p);
        p.match12 = kf.match12.data(); p.match21 = NULL;
        pairs.push_back(p); which.push_back(i);
    }
    std::vector<int32_t> nm;
    if (!SearchPairs(pairs, /*strict_th=*/1, nnratio, checkOri, nm)) return false;
    vnMatches.assign(nKFs, -1);
    vvpMapPointMatches.resize(nKFs);
    for (size_t k = 0; k < pairs.size(); ++k) {
        const FlatKeyFrame &kf = *kfs[k];
        std::vector<MapPoint*> &vpMatches12 = vvpMapPointMatches[which[k]];
        vpMatches12 = std::vector<MapPoint*>(cur.vpMapPoints.size(), static_cast<MapPoint*>(NULL));
        for (int i = 0; i < cur.N; ++i)
            if (kf.match12[i] >= 0) vpMatches12[i] = kf.vpMapPoints[kf.match12[i]];                    // ORBmatcher.cc:803
        vnMatches[which[k]] = nm[k];
    }
    return true;
}

} // namespace ORB_SLAM2
