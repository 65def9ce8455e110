// ORBmatcher::FuseKeyFrames / FuseKeyFramesSim3 of include/orbslam_hip.hpp (fuseKeyFramesWith) on a toy map of several keyframes,
// with a stub candidate stage that answers from a file; driven by tests/test_cpu_fuse_keyframes.py.  No device call is made.
// The file (all integers):
//   sim3 npoints nkf K m
//   per keyframe, ascending id:  id n / desc[n][32] / stereo[n] (mvuRight >= 0) / slots[n] (handle or -1)
//   per map point:               bad nobs {kf idx} ... / desc[32]
//   the K target ids / the list[m] (handle or -1)
//   ncalls, then per call of the candidate stage, in order:  Kc nd / points[nd] / desc[nd][32] / active[Kc][nd] /
//                                                            Kc nd / best[Kc][nd] / idx[Kc][nd] / visible[Kc][nd]
// The toy map restates what tests/fuse_keyframes_reference.py restates (MapPoint::AddObservation, Replace with its
// IsInKeyFrame branch and ComputeDistinctiveDescriptors, KeyFrame::AddMapPoint, GetMapPoints); a keyframe's id stands for its
// address in the order of mObservations.  The stub checks that every call asks for the recorded points, descriptors and mask.
// Output: nFused per target / waits refreshes / the ops {kind k a b}: 0 add (h, idx), 1 replace (dead, heir), 2 record (i, h),
// 3 the caller's replace (dead, heir).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "orbslam_hip.hpp"

using namespace orbslam_hip;

static FILE *g_in;
static int rd()
{
    int v;
    if (fscanf(g_in, "%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
static void fail(const char *what) { fprintf(stderr, "%s\n", what); exit(3); }

struct ToyKF { std::vector<uint8_t> desc; std::vector<int> stereo, slots; };

struct World {
    std::map<int, ToyKF> kfs;
    std::vector<int> bad, nobs;
    std::vector<std::map<int, int>> obs;            // mObservations: keyframe id -> keypoint index
    std::vector<uint8_t> desc;                      // mDescriptor, 32 bytes each
    std::vector<int> targets, list, ops;
    bool sim3 = false;
    int k = -1;
    std::set<int> already;                          // spAlreadyFound of the current target
    std::map<int, int> rep;                         // vpReplacePoints of the current target

    void addObservation(int h, int kf, int idx)     // MapPoint.cc:113-132
    {
        if (obs[h].count(kf)) return;
        obs[h][kf] = idx;
        nobs[h] += kfs[kf].stereo[idx] ? 2 : 1;
    }
    void computeDistinctive(int h)                  // MapPoint.cc:305-370
    {
        if (bad[h] || obs[h].empty()) return;
        std::vector<const uint8_t *> rows;
        for (const auto &o : obs[h]) rows.push_back(&kfs[o.first].desc[(size_t)32 * o.second]);
        const size_t N = rows.size();
        std::vector<std::vector<int>> D(N, std::vector<int>(N, 0));
        for (size_t i = 0; i < N; ++i)
            for (size_t j = i + 1; j < N; ++j) {
                int d = 0;
                for (int b = 0; b < 32; ++b) d += __builtin_popcount(rows[i][b] ^ rows[j][b]);
                D[i][j] = D[j][i] = d;
            }
        int bestMedian = INT_MAX, bestIdx = 0;
        for (size_t i = 0; i < N; ++i) {
            std::vector<int> v(D[i]);
            std::sort(v.begin(), v.end());
            const int median = v[(size_t)(0.5 * (N - 1))];
            if (median < bestMedian) { bestMedian = median; bestIdx = (int)i; }
        }
        std::copy(rows[bestIdx], rows[bestIdx] + 32, &desc[(size_t)32 * h]);
    }
    void replacePoint(int dead, int heir)           // MapPoint.cc:240-278: dead->Replace(heir)
    {
        if (dead == heir) return;
        std::map<int, int> o;
        o.swap(obs[dead]);
        bad[dead] = 1;
        for (const auto &e : o) {
            if (!obs[heir].count(e.first)) { kfs[e.first].slots[e.second] = heir; addObservation(heir, e.first, e.second); }
            else kfs[e.first].slots[e.second] = -1;
        }
        computeDistinctive(heir);
    }
    std::set<int> mapPoints(int kf)                 // KeyFrame.cc:274-287
    {
        std::set<int> s;
        for (int h : kfs[kf].slots)
            if (h >= 0 && !bad[h]) s.insert(h);
        return s;
    }

    // ---- what FuseKeyFrames asks of the map
    int kf() const { return targets[k]; }
    int at(int i) const { return list[i]; }
    bool null(int h) const { return h < 0; }
    bool isBad(int h) const { return bad[h] != 0; }
    bool isInKeyFrame(int h) { return obs[h].count(kf()) != 0; }
    bool alreadyFound(int h) const { return already.count(h) != 0; }
    int slotOwner(int idx) { return kfs[kf()].slots[idx]; }
    int observations(int h) const { return nobs[h]; }
    const uint8_t *descriptor(int h) const { return &desc[(size_t)32 * h]; }
    bool inTarget(int h, int t) { return sim3 ? mapPoints(targets[t]).count(h) != 0 : obs[h].count(targets[t]) != 0; }
    void replace(int dead, int heir) { ops.insert(ops.end(), {1, k, dead, heir}); replacePoint(dead, heir); }
    void add(int h, int idx)
    {
        ops.insert(ops.end(), {0, k, h, idx});
        addObservation(h, kf(), idx); kfs[kf()].slots[idx] = h;
    }
    void recordReplace(int i, int h) { ops.insert(ops.end(), {2, k, i, h}); rep[i] = h; }
    void beginTarget(int t)
    {
        k = t;
        if (sim3) { already = mapPoints(kf()); rep.clear(); }
    }
    template <class Report> void endTarget(int t, Report report)
    {
        if (!sim3) return;
        for (const auto &e : rep) {                 // LoopClosing.cc:604-611
            ops.insert(ops.end(), {3, t, e.second, list[e.first]});
            replacePoint(e.second, list[e.first]);
            report(e.first);
        }
    }
};

struct Call { int K, nd; std::vector<int> points, desc, active, best, idx, vis; };

struct Stub {
    std::vector<Call> calls;
    size_t next = 0;
    int operator()(const ORBmatcher::FuseTargetView *, int K, const std::vector<int> &points, const uint8_t *desc, const uint8_t *active,
                   int32_t *best, int32_t *idx, orbm_projected_point *proj)
    {
        if (next >= calls.size()) fail("more candidate calls than recorded");
        const Call &c = calls[next++];
        if (c.K != K || c.nd != (int)points.size()) fail("a candidate call of another shape than recorded");
        for (int j = 0; j < c.nd; ++j) {
            if (c.points[j] != points[j]) fail("a candidate call for other points than recorded");
            for (int b = 0; b < 32; ++b)
                if (c.desc[32 * j + b] != desc[32 * j + b]) fail("a candidate call with other descriptors than recorded");
        }
        for (int j = 0; j < K * c.nd; ++j) {
            if ((c.active[j] != 0) != (active[j] != 0)) fail("a candidate call with another mask than recorded");
            best[j] = c.best[j]; idx[j] = c.idx[j];
            proj[j] = orbm_projected_point(); proj[j].visible = c.vis[j];
        }
        return 1;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2 || !(g_in = fopen(argv[1], "r"))) return 2;
    World w;
    w.sim3 = rd() != 0;
    const int npoints = rd(), nkf = rd(), K = rd(), m = rd();
    for (int a = 0; a < nkf; ++a) {
        const int id = rd(), n = rd();
        ToyKF &kf = w.kfs[id];
        kf.desc.resize((size_t)32 * n); kf.stereo.resize(n); kf.slots.resize(n);
        for (auto &v : kf.desc) v = (uint8_t)rd();
        for (auto &v : kf.stereo) v = rd();
        for (auto &v : kf.slots) v = rd();
    }
    w.bad.resize(npoints); w.nobs.assign(npoints, 0); w.obs.resize(npoints); w.desc.resize((size_t)32 * npoints);
    for (int h = 0; h < npoints; ++h) {
        w.bad[h] = rd();
        const int no = rd();
        for (int a = 0; a < no; ++a) { const int kf = rd(), idx = rd(); w.addObservation(h, kf, idx); }
        for (int b = 0; b < 32; ++b) w.desc[(size_t)32 * h + b] = (uint8_t)rd();
    }
    w.targets.resize(K); for (auto &v : w.targets) v = rd();
    w.list.resize(m); for (auto &v : w.list) v = rd();
    Stub stub;
    stub.calls.resize(rd());
    for (Call &c : stub.calls) {
        c.K = rd(); c.nd = rd();
        auto fill = [](std::vector<int> &v, size_t n) { v.resize(n); for (auto &x : v) x = rd(); };
        fill(c.points, c.nd); fill(c.desc, (size_t)32 * c.nd); fill(c.active, (size_t)c.K * c.nd);
        if (rd() != c.K || rd() != c.nd) fail("rows of another shape than their call");
        fill(c.best, (size_t)c.K * c.nd); fill(c.idx, (size_t)c.K * c.nd); fill(c.vis, (size_t)c.K * c.nd);
    }
    std::vector<uint8_t> ldesc((size_t)32 * m, 0);
    for (int i = 0; i < m; ++i)
        if (w.list[i] >= 0) std::copy(w.descriptor(w.list[i]), w.descriptor(w.list[i]) + 32, &ldesc[(size_t)32 * i]);
    ORBmatcher::MapPointArrays mps;
    mps.descriptors = ldesc.data(); mps.n = m;     // positions and the rest are the candidate stage's business: the stub reads none
    std::vector<ORBmatcher::FuseTargetView> targets((size_t)K);
    ORBmatcher matcher(0.8f);
    const std::vector<int> n = matcher.fuseKeyFramesWith(stub, targets, mps, w.sim3, w);
    if (stub.next != stub.calls.size()) fail("fewer candidate calls than recorded");
    for (int v : n) printf("%d ", v);
    printf("\n%d %d\n", matcher.LastFuseKeyFramesWaits(), matcher.LastFuseKeyFramesRefreshes());
    for (size_t o = 0; o + 3 < w.ops.size(); o += 4) printf("%d %d %d %d\n", w.ops[o], w.ops[o + 1], w.ops[o + 2], w.ops[o + 3]);
    return 0;
}
