// orbslam_hip::KeyFrameDatabase (include/orbslam_hip.hpp) driven by a case in the format of tests/kfdb_oracle.cc (the operations
// N, G, A, E, C, S, L, R, F), printing what the oracle prints for them, so tests/test_cxx_kfdb.py can compare the two outputs line
// by line.  (The oracle's "W" line, the list of keyframes sharing words, is internal to the class: it is printed empty.)
// Two more operations serve tools/kfdb_time.py: "B path" adds the rows of a binary file, "TR reps <bow>" prints the median
// microseconds of DetectRelocalizationCandidates (query call + host half, no covisibility graph) over reps runs with fresh ids.
// Without a device the first add fails: "NODEVICE" and exit status 3.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "orbslam_hip.hpp"

static char *cur;
static long next_int() { return strtol(cur, &cur, 10); }
static double next_double() { return strtod(cur, &cur); }
static orbslam_hip::DBoW2::BowVector next_bow()
{
    orbslam_hip::DBoW2::BowVector b;
    const long n = next_int();
    for (long i = 0; i < n; ++i) { const unsigned w = (unsigned)next_int(); b[w] = next_double(); }
    return b;
}

int main(int argc, char **argv)
{
    FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    orbslam_hip::KeyFrameDatabase *db = nullptr;
    std::map<int, std::vector<int>> graph;
    auto best = [&graph](int slot, std::vector<int> &out) { out = graph[slot]; };
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, in) > 0) {
        cur = line;
        std::string op;
        while (*cur && *cur != ' ' && *cur != '\n') op += *cur++;
        if (op.empty()) continue;
        if (op == "N") {
            db = new orbslam_hip::KeyFrameDatabase((int)next_int());
            if (db->status() != ORBX_OK) return 2;
        } else if (op == "G") {
            std::vector<int> &g = graph[(int)next_int()];
            g.clear();
            for (long n = next_int(); n > 0; --n) g.push_back((int)next_int());
        } else if (op == "A") {
            const int slot = db->add(next_bow());
            if (slot < 0) {
                if (db->status() == ORBX_ERR_NO_DEVICE) { printf("NODEVICE\n"); return 3; }
                fprintf(stderr, "add: %s\n", orbx_last_error());
                return 2;
            }
            printf("A %d\n", slot);
        } else if (op == "B") {
            while (*cur == ' ') ++cur;
            std::string path(cur);
            while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
            FILE *f = fopen(path.c_str(), "rb");
            int32_t K = 0;
            if (!f || fread(&K, 4, 1, f) != 1) return 2;
            for (int r = 0; r < K; ++r) {
                int32_t n = 0;
                if (fread(&n, 4, 1, f) != 1) return 2;
                std::vector<int32_t> w(n); std::vector<double> v(n);
                if (n && (fread(w.data(), 4, n, f) != (size_t)n || fread(v.data(), 8, n, f) != (size_t)n)) return 2;
                orbslam_hip::DBoW2::BowVector b;
                for (int i = 0; i < n; ++i) b[(unsigned)w[i]] = v[i];
                if (db->add(b) < 0) { fprintf(stderr, "add: %s\n", orbx_last_error()); return 2; }
            }
            fclose(f);
            printf("B %d\n", K);
        } else if (op == "TR") {
            const long reps = next_int();
            const orbslam_hip::DBoW2::BowVector q = next_bow();
            std::vector<double> t;
            size_t sink = 0;
            for (long r = -3; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                sink += db->DetectRelocalizationCandidates(q, 1000000000ul + (long unsigned)(r + 3), best).size();
                if (r >= 0) t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            }
            if (db->status() != ORBX_OK) return 2;
            std::sort(t.begin(), t.end());
            printf("TR %.3f %zu\n", t[t.size() / 2], sink);
        } else if (op == "E") {
            db->erase((int)next_int());
            if (db->status() != ORBX_OK) return 2;
        } else if (op == "C") {
            db->clear(); graph.clear();
        } else if (op == "S") {
            std::vector<int32_t> list;
            for (long n = next_int(); n > 0; --n) list.push_back((int32_t)next_int());
            printf("S 1 %a\n", (double)db->MinScore(next_bow(), list));
            if (db->status() != ORBX_OK) return 2;
        } else if (op == "L" || op == "R") {
            const long unsigned id = (long unsigned)next_int();
            std::vector<int> connected, c;
            float minScore = 0;
            if (op == "L") {
                minScore = (float)next_double();
                for (long n = next_int(); n > 0; --n) connected.push_back((int)next_int());
                c = db->DetectLoopCandidates(next_bow(), id, connected, minScore, best);
            } else {
                c = db->DetectRelocalizationCandidates(next_bow(), id, best);
            }
            if (db->status() != ORBX_OK) { fprintf(stderr, "query: %s\n", orbx_last_error()); return 2; }
            printf("%s %zu", op.c_str(), c.size());
            for (int s : c) printf(" %d", s);
            printf("\nW 0\n");
        } else if (op == "F") {
            printf("F %d\n", db->slots());
            for (int s = 0; s < db->slots(); ++s) {
                const orbslam_hip::KeyFrameDatabase::Fields &f = db->fields(s);
                printf("%lu %d %a %lu %d %a\n", f.mnLoopQuery, f.mnLoopWords, (double)f.mLoopScore, f.mnRelocQuery, f.mnRelocWords, (double)f.mRelocScore);
            }
        } else {
            return 2;
        }
    }
    delete db;
    printf("OK\n");
    return 0;
}
