// integration/Initializer_hip.cc -- Initializer::Initialize, ::ReconstructF and ::CheckRT (include/Initializer.h,
// src/Initializer.cc:44-121, :470-570, :798-907) over orbm_init_find_models, orbm_init_reconstruct_f and orbm_init_check_rt.
//
// Goes to src/Initializer_hip.cc BESIDE src/Initializer.cc in the reference's CMakeLists.txt: the reference's file stays, with its
// definitions of these three methods (and of FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography,
// CheckFundamental, Normalize, Triangulate and DecomposeE, which nothing calls any more) put between
//     #ifndef ORBSLAM_HIP_INITIALIZER   ...   #endif
// and ORBSLAM_HIP_INITIALIZER defined for the build.  The constructor and ReconstructH (:572-732) stay the reference's.  Like the
// other shells this file cannot be compiled where OpenCV / DBoW2 are absent, and reference.patch does not carry it or the #ifndef
// (its hunks are pinned); the class keeps its header.
//
//   Initialize     the thread pair of :99-109 becomes ONE orbm_init_find_models call (all 2 x mMaxIterations hypotheses in one
//                  launch); DUtils::Random::RandomInt after SeedRandOnce(0) stays the source of the draws, in the order of :82-97.
//   ReconstructF   one orbm_init_reconstruct_f call: the four CheckRT passes are one launch.
//   CheckRT        a one-motion orbm_init_check_rt.  Its caller is the reference's own ReconstructH, which this fork takes only at
//                  RH > 0.99 (:115; upstream has 0.40): its eight CheckRT calls are served one at a time.
// One difference to the reference: when no fundamental matrix scores above 0 the reference leaves vbMatchesInliersF empty and F21 an
// empty cv::Mat, and ReconstructF throws inside cv::Mat arithmetic; here Initialize returns false.
#include "Initializer.h"

#include <iostream>

#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbslam_hip.h"

namespace ORB_SLAM2
{

namespace
{
void FlatKeys(const vector<cv::KeyPoint> &v, vector<float> &out)
{
    out.resize(2 * v.size() + 2);
    for (size_t i = 0; i < v.size(); ++i) { out[2 * i] = v[i].pt.x; out[2 * i + 1] = v[i].pt.y; }
}

void FlatMatches(const vector<pair<int, int> > &v, vector<int32_t> &out)
{
    out.resize(2 * v.size() + 2);
    for (size_t i = 0; i < v.size(); ++i) { out[2 * i] = v[i].first; out[2 * i + 1] = v[i].second; }
}

void FlatFlags(const vector<bool> &v, size_t n, vector<uint8_t> &out)
{
    out.assign(n + 1, 0);
    for (size_t i = 0; i < n && i < v.size(); ++i) out[i] = v[i] ? 1 : 0;
}

void FlatMat(const cv::Mat &m, float *out)
{
    for (int r = 0; r < m.rows; ++r)
        for (int c = 0; c < m.cols; ++c) out[m.cols * r + c] = m.at<float>(r, c);
}

cv::Mat ToMat(const float *v, int rows, int cols)
{
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<float>(r, c) = v[cols * r + c];
    return m;
}

void UnpackMask(const vector<uint64_t> &words, size_t n, vector<bool> &out)
{
    out.assign(n, false);
    for (size_t i = 0; i < n; ++i) out[i] = (words[i / 64] >> (i % 64)) & 1;
}
}

bool Initializer::Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated)
{
    // :47-63
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(make_pair(i, vMatches12[i]));
            mvbMatched1[i] = true;
        } else
            mvbMatched1[i] = false;
    }
    const int N = mvMatches12.size();

    // :65-97: the sets of all iterations, drawn as the reference draws them
    vector<size_t> vAllIndices;
    vAllIndices.reserve(N);
    vector<size_t> vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets = vector<vector<size_t> >(mMaxIterations, vector<size_t>(8, 0));
    DUtils::Random::SeedRandOnce(0);
    vector<int32_t> sets(8 * (size_t)mMaxIterations + 8);
    for (int it = 0; it < mMaxIterations; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
            int idx = vAvailableIndices[randi];
            mvSets[it][j] = idx;
            sets[8 * it + j] = idx;
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    // :99-109: both models, every hypothesis, one launch
    vector<float> keys1, keys2;
    vector<int32_t> matches;
    FlatKeys(mvKeys1, keys1); FlatKeys(mvKeys2, keys2); FlatMatches(mvMatches12, matches);
    const size_t words = ((size_t)N + 63) / 64;
    vector<uint64_t> maskH(words + 1, 0), maskF(words + 1, 0);
    orbm_init_models models;
    const int rc = orbm_init_find_models(keys1.data(), (int)mvKeys1.size(), keys2.data(), (int)mvKeys2.size(), matches.data(), N, sets.data(),
                                         mMaxIterations, mSigma, &models, maskH.data(), maskF.data(), NULL, NULL, NULL);
    if (rc != ORBX_OK) {
        std::cerr << "Initializer: " << orbx_last_error() << std::endl;
        return false;
    }
    vector<bool> vbMatchesInliersH, vbMatchesInliersF;
    UnpackMask(maskH, N, vbMatchesInliersH);
    UnpackMask(maskF, N, vbMatchesInliersF);
    cv::Mat H = ToMat(models.H21, 3, 3), F = ToMat(models.F21, 3, 3);
    const float SH = models.SH, SF = models.SF;

    // :111-118
    float RH = SH / (SH + SF);
    if (RH > 0.99)
        return ReconstructH(vbMatchesInliersH, H, mK, R21, t21, vP3D, vbTriangulated, 1.0, 50);   // the reference's own
    if (models.itF < 0)
        return false;                                            // no fundamental matrix: the reference throws in ReconstructF here
    return ReconstructF(vbMatchesInliersF, F, mK, R21, t21, vP3D, vbTriangulated, 0.95, 60);
}

bool Initializer::ReconstructF(vector<bool> &vbMatchesInliers, cv::Mat &F21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21,
                               vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated, float minParallax, int minTriangulated)
{
    vector<float> keys1, keys2;
    vector<int32_t> matches;
    vector<uint8_t> inliers;
    FlatKeys(mvKeys1, keys1); FlatKeys(mvKeys2, keys2); FlatMatches(mvMatches12, matches);
    FlatFlags(vbMatchesInliers, mvMatches12.size(), inliers);
    float f[9], k[9];
    FlatMat(F21, f); FlatMat(K, k);
    const size_t n1 = mvKeys1.size();
    vector<float> p3d(3 * n1 + 3);
    vector<uint8_t> tri(n1 + 1);
    orbm_init_reconstruction rec;
    const int rc = orbm_init_reconstruct_f(keys1.data(), (int)n1, keys2.data(), (int)mvKeys2.size(), matches.data(), (int)mvMatches12.size(),
                                           inliers.data(), f, k, mSigma, minParallax, minTriangulated, &rec, p3d.data(), tri.data());
    R21 = cv::Mat();
    t21 = cv::Mat();
    if (rc != ORBX_OK) {
        std::cerr << "Initializer: " << orbx_last_error() << std::endl;
        return false;
    }
    if (!rec.found) return false;
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; ++i) {
        vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
    R21 = ToMat(rec.R21, 3, 3);
    t21 = ToMat(rec.t21, 3, 1);
    return true;
}

int Initializer::CheckRT(const cv::Mat &R, const cv::Mat &t, const vector<cv::KeyPoint> &vKeys1, const vector<cv::KeyPoint> &vKeys2,
                         const vector<Match> &vMatches12, vector<bool> &vbMatchesInliers, const cv::Mat &K, vector<cv::Point3f> &vP3D,
                         float th2, vector<bool> &vbGood, float &parallax)
{
    vector<float> keys1, keys2;
    vector<int32_t> matches;
    vector<uint8_t> inliers;
    FlatKeys(vKeys1, keys1); FlatKeys(vKeys2, keys2); FlatMatches(vMatches12, matches);
    FlatFlags(vbMatchesInliers, vMatches12.size(), inliers);
    float r[9], tv[3], k[9];
    FlatMat(R, r); FlatMat(t, tv); FlatMat(K, k);
    const size_t n1 = vKeys1.size();
    vector<float> p3d(3 * n1 + 3);
    vector<uint8_t> good(n1 + 1);
    int32_t nGood = 0;
    parallax = 0;
    vbGood = vector<bool>(n1, false);
    vP3D.resize(n1);
    const int rc = orbm_init_check_rt(keys1.data(), (int)n1, keys2.data(), (int)vKeys2.size(), matches.data(), (int)vMatches12.size(),
                                      inliers.data(), k, r, tv, 1, th2, good.data(), p3d.data(), NULL, NULL, &nGood, &parallax);
    if (rc != ORBX_OK) {
        std::cerr << "Initializer: " << orbx_last_error() << std::endl;
        return 0;
    }
    for (size_t i = 0; i < n1; ++i) {
        vbGood[i] = good[i] != 0;
        vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);     // (the reference leaves unwritten entries as they were)
    }
    return nGood;
}

} // namespace ORB_SLAM2
