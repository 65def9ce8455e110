// kfdb_oracle.cc -- KeyFrameDatabase as the reference runs it (src/KeyFrameDatabase.cc:40-309, src/LoopClosing.cc:127-138,
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), restated in this project's own words over the same containers (std::map /
// std::list / std::vector), with the same loop order and number types, for the tests (g++ -O2 -ffp-contract=off: against tests/kfdb_reference.py and the device) and as the CPU
// baseline of tools/kfdb_time.py (-O3 -march=native).  A keyframe is known by its slot: the order of add, restarting after clear.
// mLoopScore / mRelocScore, which the reference leaves uninitialised, start at 0.0f.
//
// Reads a case from the file named on the command line, or from stdin; one operation per line, numbers as strtod reads them (values
// are written as hex floats); a BowVector is "n w1 v1 .. wn vn":
//   N nwords                               first line
//   G slot k s1 .. sk                      GetBestCovisibilityKeyFrames(10) of slot, as slots
//   A <bow>                                add                                          -> "A slot"
//   B path                                 add every row of a binary file (int32 K, then per row int32 n, int32 ids[n], double values[n])
//                                                                                       -> "B K microseconds-per-add"
//   E slot / C                             erase / clear
//   Q <bow>                                what a query finds, no field touched         -> "Q K" then K x "common first score"
//   S k s1 .. sk <bow>                     DetectLoop's score loop                      -> "S k score .."
//   L id minScore nc c1 .. cnc <bow>       DetectLoopCandidates (c: connected slots)    -> "L k cand .." and "W k slot .." (lKFsSharingWords)
//   R id <bow>                             DetectRelocalizationCandidates               -> "R k cand .." and "W k slot .."
//   F                                      the six persistent fields of every slot      -> "F K" then K x six numbers
//   TR reps <bow> / TS reps k s1 .. sk <bow>   median microseconds of R (fresh ids, no output) / of S over reps runs -> "TR us" / "TS us"
// Scores are printed with %a.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

typedef std::map<unsigned, double> BowVector;      // DBoW2::BowVector: std::map<WordId, WordValue>

struct KeyFrame {
    int slot;
    BowVector mBowVec;
    bool alive = true;
    long unsigned mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0.0f;
    long unsigned mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0.0f;
    std::vector<KeyFrame *> best;                  // GetBestCovisibilityKeyFrames(10)
};

// L1 score of two BowVectors: over the words both hold, in ascending word id, sum |a - b| - |a| - |b| in double; the result is
// -sum / 2 (-0.0 when nothing is shared).  A side that is behind jumps with lower_bound, as the reference does.
static double score(const BowVector &qa, const BowVector &kb)
{
    double sum = 0;
    BowVector::const_iterator a = qa.begin(), b = kb.begin();
    while (a != qa.end() && b != kb.end()) {
        if (a->first < b->first) { a = qa.lower_bound(b->first); continue; }
        if (b->first < a->first) { b = kb.lower_bound(a->first); continue; }
        sum += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second);
        ++a; ++b;
    }
    return -sum / 2.0;
}

struct Database {
    std::vector<std::list<KeyFrame *>> inverted;   // per word: the keyframes holding it, in the order of add
    std::vector<KeyFrame *> kfs;
    std::vector<int> sharing;                      // slots of the last query's list of keyframes sharing words

    void add(KeyFrame *kf)
    {
        for (const auto &wv : kf->mBowVec) inverted[wv.first].push_back(kf);
    }
    void erase(KeyFrame *kf)
    {
        for (const auto &wv : kf->mBowVec) {
            std::list<KeyFrame *> &l = inverted[wv.first];
            std::list<KeyFrame *>::iterator it = std::find(l.begin(), l.end(), kf);
            if (it != l.end()) l.erase(it);        // the others keep their order
        }
        kf->alive = false;
    }
    void clear()
    {
        const size_t n = inverted.size();
        inverted.clear();
        inverted.resize(n);
        for (KeyFrame *k : kfs) delete k;
        kfs.clear();
    }

    // Both queries (src/KeyFrameDatabase.cc:76-197 loop form, :199-309 relocalisation form), the fields of the form chosen by
    // member pointers.  Differences of the loop form: connected keyframes are never listed (their count restarts at every meeting),
    // scores below minScore are dropped after being stored, the best total starts at minScore, and a neighbour must pass the word
    // cut as well as carry this query's id.
    std::vector<KeyFrame *> Detect(bool loop, const BowVector &bow, long unsigned id, const std::set<KeyFrame *> &connected, float minScore)
    {
        long unsigned KeyFrame::*qid = loop ? &KeyFrame::mnLoopQuery : &KeyFrame::mnRelocQuery;
        int KeyFrame::*nw = loop ? &KeyFrame::mnLoopWords : &KeyFrame::mnRelocWords;
        float KeyFrame::*sc = loop ? &KeyFrame::mLoopScore : &KeyFrame::mRelocScore;
        std::list<KeyFrame *> listed;
        for (const auto &wv : bow)
            for (KeyFrame *k : inverted[wv.first]) {
                if (k->*qid != id) {
                    k->*nw = 0;
                    if (!loop || !connected.count(k)) { k->*qid = id; listed.push_back(k); }
                }
                ++(k->*nw);
            }
        sharing.clear();
        for (KeyFrame *k : listed) sharing.push_back(k->slot);
        std::vector<KeyFrame *> out;
        if (listed.empty()) return out;
        int most = 0;
        for (KeyFrame *k : listed) most = std::max(most, k->*nw);
        const int cut = most * 0.8f;
        std::list<std::pair<float, KeyFrame *>> kept, groups;
        for (KeyFrame *k : listed)
            if (k->*nw > cut) {
                const float si = score(bow, k->mBowVec);
                k->*sc = si;
                if (!loop || si >= minScore) kept.push_back(std::make_pair(si, k));
            }
        if (kept.empty()) return out;
        float bestTotal = loop ? minScore : 0.0f;
        for (const auto &sk : kept) {
            float total = sk.first, top = sk.first;
            KeyFrame *winner = sk.second;
            for (KeyFrame *n : sk.second->best) {
                if (n->*qid != id || (loop && !(n->*nw > cut))) continue;
                total += n->*sc;
                if (n->*sc > top) { winner = n; top = n->*sc; }
            }
            groups.push_back(std::make_pair(total, winner));
            if (total > bestTotal) bestTotal = total;
        }
        const float keepAbove = 0.75f * bestTotal;
        std::set<KeyFrame *> seen;
        for (const auto &g : groups)
            if (g.first > keepAbove && seen.insert(g.second).second) out.push_back(g.second);
        return out;
    }
    std::vector<KeyFrame *> DetectLoopCandidates(const BowVector &bow, long unsigned id, const std::set<KeyFrame *> &connected, float minScore)
    {
        return Detect(true, bow, id, connected, minScore);
    }
    std::vector<KeyFrame *> DetectRelocalizationCandidates(const BowVector &bow, long unsigned id)
    {
        return Detect(false, bow, id, std::set<KeyFrame *>(), 0.0f);
    }
};

// ---------------------------------------------------------------------------------------------------------------- the case reader
static char *cur;
static long next_int() { return strtol(cur, &cur, 10); }
static double next_double() { return strtod(cur, &cur); }
static BowVector next_bow()
{
    BowVector b;
    const long n = next_int();
    for (long i = 0; i < n; ++i) { const unsigned w = (unsigned)next_int(); b[w] = next_double(); }
    return b;
}
static double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv)
{
    FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Database db;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, in) > 0) {
        cur = line;
        while (*cur == ' ') ++cur;
        std::string op;
        while (*cur && *cur != ' ' && *cur != '\n') op += *cur++;
        if (op.empty()) continue;
        if (op == "N") {
            db.inverted.resize((size_t)next_int());
        } else if (op == "G") {
            KeyFrame *k = db.kfs.at(next_int());
            k->best.clear();
            for (long n = next_int(); n > 0; --n) k->best.push_back(db.kfs.at(next_int()));
        } else if (op == "A") {
            KeyFrame *k = new KeyFrame();
            k->slot = (int)db.kfs.size();
            k->mBowVec = next_bow();
            db.kfs.push_back(k);
            db.add(k);
            printf("A %d\n", k->slot);
        } else if (op == "B") {
            while (*cur == ' ') ++cur;
            std::string path(cur);
            while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
            FILE *f = fopen(path.c_str(), "rb");
            int32_t K = 0;
            if (!f || fread(&K, 4, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
            double spent = 0;
            for (int r = 0; r < K; ++r) {
                int32_t n = 0;
                if (fread(&n, 4, 1, f) != 1) return 2;
                std::vector<int32_t> w(n); std::vector<double> v(n);
                if (n && (fread(w.data(), 4, n, f) != (size_t)n || fread(v.data(), 8, n, f) != (size_t)n)) return 2;
                KeyFrame *k = new KeyFrame();
                k->slot = (int)db.kfs.size();
                for (int i = 0; i < n; ++i) k->mBowVec[(unsigned)w[i]] = v[i];      // (the keyframe has its BowVector before add, as in the reference)
                db.kfs.push_back(k);
                const double t0 = now_us();
                db.add(k);
                spent += now_us() - t0;
            }
            fclose(f);
            printf("B %d %.3f\n", K, K ? spent / K : 0.0);
        } else if (op == "E") {
            db.erase(db.kfs.at(next_int()));
        } else if (op == "C") {
            db.clear();
        } else if (op == "Q") {
            const BowVector q = next_bow();
            std::vector<int> common(db.kfs.size(), 0), first(db.kfs.size(), -1);
            int i = 0;
            for (BowVector::const_iterator vit = q.begin(); vit != q.end(); vit++, i++)
                for (KeyFrame *k : db.inverted[vit->first]) {
                    if (!common[k->slot]) first[k->slot] = i;
                    common[k->slot]++;
                }
            printf("Q %zu\n", db.kfs.size());
            for (KeyFrame *k : db.kfs) {
                const float si = k->alive ? (float)score(q, k->mBowVec) : 0.0f;
                printf("%d %d %a\n", k->alive ? common[k->slot] : -1, first[k->slot], (double)si);
            }
        } else if (op == "S" || op == "TS") {
            const long reps = op == "TS" ? next_int() : 1;
            std::vector<KeyFrame *> list;
            for (long n = next_int(); n > 0; --n) list.push_back(db.kfs.at(next_int()));
            const BowVector q = next_bow();
            std::vector<float> out(list.size());
            std::vector<double> t;
            for (long r = 0; r < reps; ++r) {
                const double t0 = now_us();
                for (size_t i = 0; i < list.size(); ++i) out[i] = score(q, list[i]->mBowVec);
                t.push_back(now_us() - t0);
            }
            if (op == "TS") { printf("TS %.3f\n", median(t)); continue; }
            printf("S %zu", out.size());
            for (float s : out) printf(" %a", (double)s);
            printf("\n");
        } else if (op == "L" || op == "R") {
            const long unsigned id = (long unsigned)next_int();
            std::set<KeyFrame *> connected;
            float minScore = 0;
            if (op == "L") {
                minScore = (float)next_double();
                for (long n = next_int(); n > 0; --n) connected.insert(db.kfs.at(next_int()));
            }
            const BowVector q = next_bow();
            const std::vector<KeyFrame *> c = op == "L" ? db.DetectLoopCandidates(q, id, connected, minScore) : db.DetectRelocalizationCandidates(q, id);
            printf("%s %zu", op.c_str(), c.size());
            for (KeyFrame *k : c) printf(" %d", k->slot);
            printf("\nW %zu", db.sharing.size());
            for (int s : db.sharing) printf(" %d", s);
            printf("\n");
        } else if (op == "TR") {
            const long reps = next_int();
            const BowVector q = next_bow();
            std::vector<double> t;
            size_t sink = 0;
            for (long r = 0; r < reps; ++r) {
                const double t0 = now_us();
                sink += db.DetectRelocalizationCandidates(q, 1000000000ul + (long unsigned)r).size();
                t.push_back(now_us() - t0);
            }
            printf("TR %.3f %zu\n", median(t), sink);
        } else if (op == "F") {
            printf("F %zu\n", db.kfs.size());
            for (KeyFrame *k : db.kfs)
                printf("%lu %d %a %lu %d %a\n", k->mnLoopQuery, k->mnLoopWords, (double)k->mLoopScore, k->mnRelocQuery, k->mnRelocWords,
                       (double)k->mRelocScore);
        } else {
            fprintf(stderr, "unknown operation %s\n", op.c_str());
            return 2;
        }
    }
    free(line);
    return 0;
}
