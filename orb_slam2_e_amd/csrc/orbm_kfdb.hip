// orbm_kfdb.hip -- KeyFrameDatabase on the device (src/KeyFrameDatabase.cc:40-309, src/LoopClosing.cc:120-141,
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  The store keeps the BowVector of every added keyframe in HBM as
// one row of (word id, value) under a slot number handed out in the order of add; a query is ONE launch in which a wave per
// keyframe looks every word of its row up in the query (held in LDS) and leaves the number of shared words, the query index of the
// first shared word and the L1 score -- the double sum taken in ascending word order, as L1Scoring::score takes it -- for every
// slot.  What the reference does with those numbers (the list order, the 0.8 cut, the covisibility fold) is host work over
// pointer graphs and stays with the caller (orb_slam2_e_amd/keyframe_database.py, orbslam_hip::KeyFrameDatabase).
#include <algorithm>
#include <mutex>

#include "orbm_internal.h"

using namespace orbm_detail;

namespace {

constexpr int KF_MAXN = 8192;            // words of a row or a query: the resident frame's keypoint limit (a BowVector has at most one word per keypoint)
constexpr int KF_WAVES = MT / 64;        // keyframes a workgroup scores at a time
constexpr int KF_CHUNKS = 4;             // 64-word chunks of a row a wave has in flight
constexpr int KF_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups: more keyframes than that are taken in strides
constexpr size_t KF_FIRST_ENTRIES = (size_t)1 << 16, KF_FIRST_SLOTS = (size_t)1 << 10;
constexpr size_t KF_MAX_ENTRIES = 0x7fffffffu;    // a row's offset is an int

std::atomic<int> g_max_blocks{0};        // orbm_debug_kfdb_max_blocks: 0 = KF_MAX_BLOCKS
std::atomic<int> g_last_kfdb_waits{0};   // host waits of the last orbm_kfdb_query / orbm_kfdb_score (orbm_debug_last_kfdb_waits)

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// One wave per keyframe i of `count` (slot list[i], or slot i when list is NULL): every lane takes a word of the row and finds its
// lower bound in the query's ascending ids (LDS, shared by the workgroup's waves and by every keyframe they stride over).  The hits
// of 64 consecutive row words are a ballot; their terms |vi - wi| - |vi| - |wi| were computed in parallel, and are ADDED one by one in lane
// order, which is ascending word order: the sum is the sequential double sum of L1Scoring::score, bit for bit.  A dead row
// (length -1) gives common -1, first -1, score +0.0f.  Workgroups share nothing and never wait for each other.
__global__ __launch_bounds__(MT) void k_kfdb_query(const int2 *__restrict__ rows, const int32_t *__restrict__ words,
                                                   const double *__restrict__ values, const int32_t *__restrict__ qw,
                                                   const double *__restrict__ qv, int nq, const int32_t *__restrict__ list, int count,
                                                   int32_t *__restrict__ common, int32_t *__restrict__ first, float *__restrict__ score)
{
    extern __shared__ int32_t sq[];      // [nq]
    for (int i = threadIdx.x; i < nq; i += MT) sq[i] = qw[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int top = 1;                         // the largest power of two <= nq (nq >= 1)
    while (top * 2 <= nq) top *= 2;
    for (int i = blockIdx.x * KF_WAVES + wave; i < count; i += gridDim.x * KF_WAVES) {
        const int slot = list ? list[i] : i;
        const int2 row = rows[slot];     // (offset, length)
        if (row.y < 0) {
            if (lane == 0) { if (common) common[i] = -1; if (first) first[i] = -1; score[i] = 0.0f; }
            continue;
        }
        double sum = 0.0;
        int ncommon = 0, nfirst = -1;
        for (int base = 0; base < row.y; base += 64 * KF_CHUNKS) {
            // KF_CHUNKS chunks of 64 words side by side: their loads leave together and their searches interleave, so a row costs
            // two dependent memory round trips per 256 words (the ids; then the values of the hits) instead of per 64.
            // Every load below is unconditional (a lane without a word, or without a hit, reads element 0 of the row or of the
            // query): with the loads under branches the compiler waits for each chunk's in turn.
            int w[KF_CHUNKS], lo[KF_CHUNKS];     // lo: number of query ids < w
            bool in[KF_CHUNKS], hit[KF_CHUNKS];
            double term[KF_CHUNKS];
#pragma unroll
            for (int u = 0; u < KF_CHUNKS; ++u) {
                const int k = base + 64 * u + lane;
                in[u] = k < row.y;
                w[u] = words[(size_t)row.x + (in[u] ? k : 0)];
                lo[u] = 0;
            }
            for (int s = top; s > 0; s >>= 1) {
#pragma unroll
                for (int u = 0; u < KF_CHUNKS; ++u) {
                    const int p = lo[u] + s;
                    lo[u] = (sq[min(p, nq) - 1] < w[u] && p <= nq) ? p : lo[u];
                }
            }
#pragma unroll
            for (int u = 0; u < KF_CHUNKS; ++u) hit[u] = (sq[min(lo[u], nq - 1)] == w[u]) && lo[u] < nq && in[u];
#pragma unroll
            for (int u = 0; u < KF_CHUNKS; ++u) {
                const double vi = qv[hit[u] ? lo[u] : 0], wi = values[(size_t)row.x + (hit[u] ? base + 64 * u + lane : 0)];
                term[u] = fabs(vi - wi) - fabs(vi) - fabs(wi);       // (read for the hits only)
            }
#pragma unroll
            for (int u = 0; u < KF_CHUNKS; ++u) {        // chunk by chunk, lane by lane: ascending word id
                unsigned long long m = __ballot(hit[u]);
                if (m) {
                    if (nfirst < 0) nfirst = __builtin_amdgcn_readlane(lo[u], __ffsll((long long)m) - 1);
                    ncommon += __popcll(m);
                    for (; m; m &= m - 1) sum += readlane_f64(term[u], __ffsll((long long)m) - 1);
                }
            }
        }
        if (lane == 0) {
            if (common) common[i] = ncommon;
            if (first) first[i] = nfirst;
            score[i] = (float)(-sum / 2.0);      // nothing shared: -0.0f
        }
    }
}

// a row from the call's staged block to the end of the pools, and its (offset, length) into the slot table
__global__ __launch_bounds__(MT) void k_kfdb_append(const int32_t *__restrict__ sw, const double *__restrict__ sv, int n,
                                                    int32_t *__restrict__ words, double *__restrict__ values, int2 *__restrict__ rows,
                                                    int slot, int off)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i < n) { words[(size_t)off + i] = sw[i]; values[(size_t)off + i] = sv[i]; }
    if (i == 0) rows[slot] = make_int2(off, n);
}

} // namespace

// Rows are appended to two pools (ids, values) and never moved inside them; a slot table holds (offset, length) per slot.  erase marks
// the slot's length -1 on both sides and leaves the row where it is: dead rows are reclaimed by clear only, which resets the fill
// marks and keeps the capacity.  A pool that is full is replaced by one of twice the size and the resident part copied over
// (reallocs counts those replacements).  Every call holds the mutex and returns after its own wait, so no launch is in flight when
// a pool is replaced.
struct orbm_kfdb {
    int nwords = 0, live = 0, reallocs = 0;
    std::mutex mu;
    std::vector<int> len;                                   // per slot: words of the row, -1 = erased
    size_t used = 0, ent_cap = 0, slot_cap = 0;             // entries in the pools, capacities
    int32_t *d_words = nullptr; double *d_values = nullptr; int2 *d_rows = nullptr;
};

namespace {

// ids strictly ascending inside [0, nwords)
bool row_ok(int nwords, const int32_t *w, int n)
{
    for (int i = 0; i < n; ++i)
        if (w[i] < 0 || w[i] >= nwords || (i && w[i] <= w[i - 1])) return false;
    return true;
}

// a block of `want` elements with the first `keep` of `p` copied over (on st, waited for); `p` is left alone
template <typename T>
int grown_copy(const T *p, size_t keep, size_t want, hipStream_t st, T **out)
{
    T *q = nullptr;
    ORBX_HIP(hipMalloc((void **)&q, sizeof(T) * want));
    if (p && keep) {
        hipError_t e = hipMemcpyAsync(q, p, sizeof(T) * keep, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(q); ORBX_HIP(e); }
    }
    *out = q;
    return ORBX_OK;
}

// room for n more entries and one more slot.  Both pools are replaced together: the new ones are made first, and only when both
// stand are the old ones freed, so a failure leaves the store as it was.
int make_room(orbm_kfdb *db, int n, hipStream_t st)
{
    const size_t need = db->used + (size_t)n, nslots = db->len.size() + 1;
    if (need > KF_MAX_ENTRIES) ORBX_FAIL(ORBX_ERR_CAPACITY, "more than 2^31 - 1 words in the database");
    if (need > db->ent_cap || !db->d_words) {
        const size_t want = std::min(std::max({need, 2 * db->ent_cap, KF_FIRST_ENTRIES}), KF_MAX_ENTRIES);
        int32_t *w = nullptr; double *v = nullptr;
        if (const int rc = grown_copy(db->d_words, db->used, want, st, &w)) return rc;
        if (const int rc = grown_copy(db->d_values, db->used, want, st, &v)) { (void)hipFree(w); return rc; }
        if (db->d_words) { (void)hipFree(db->d_words); (void)hipFree(db->d_values); db->reallocs++; }
        db->d_words = w; db->d_values = v; db->ent_cap = want;
    }
    if (nslots > db->slot_cap) {
        const size_t want = std::max({nslots, 2 * db->slot_cap, KF_FIRST_SLOTS});
        int2 *r = nullptr;
        if (const int rc = grown_copy(db->d_rows, db->len.size(), want, st, &r)) return rc;
        if (db->d_rows) { (void)hipFree(db->d_rows); db->reallocs++; }
        db->d_rows = r; db->slot_cap = want;
    }
    return ORBX_OK;
}

// what a query leaves without a launch: no live keyframe, or an empty query (nothing can be shared)
void fill_unshared(const orbm_kfdb *db, int32_t *common, int32_t *first, float *score)
{
    for (size_t s = 0; s < db->len.size(); ++s) {
        const bool dead = db->len[s] < 0;
        common[s] = dead ? -1 : 0; first[s] = -1; score[s] = dead ? 0.0f : -0.0f;
    }
}

int launch_query(const orbm_kfdb *db, StagedCall &sc, size_t o_qw, size_t o_qv, int nq, const int32_t *list, int count, int32_t *common,
                 int32_t *first, float *score)
{
    const int cap = g_max_blocks.load(std::memory_order_relaxed);
    const int blocks = std::min((count + KF_WAVES - 1) / KF_WAVES, cap > 0 ? std::min(cap, KF_MAX_BLOCKS) : KF_MAX_BLOCKS);
    hipLaunchKernelGGL(k_kfdb_query, dim3(blocks), dim3(MT), sizeof(int32_t) * (size_t)nq, sc.stream(), (const int2 *)db->d_rows,
                       (const int32_t *)db->d_words, (const double *)db->d_values, (const int32_t *)sc.d<int32_t>(o_qw),
                       (const double *)sc.d<double>(o_qv), nq, list, count, common, first, score);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

} // namespace

extern "C" {

int orbm_kfdb_create(int nwords, orbm_kfdb **out)
{
    if (!out || nwords <= 0) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    orbm_kfdb *db = new orbm_kfdb();
    db->nwords = nwords;
    *out = db;
    return ORBX_OK;
}

int orbm_kfdb_destroy(orbm_kfdb *db)
{
    if (!db) return ORBX_OK;
    if (db->d_words) (void)hipFree(db->d_words);
    if (db->d_values) (void)hipFree(db->d_values);
    if (db->d_rows) (void)hipFree(db->d_rows);
    delete db;
    return ORBX_OK;
}

int orbm_kfdb_add(orbm_kfdb *db, const int32_t *words, const double *values, int n, int32_t *slot)
{
    if (!db || !slot || n < 0 || (n && (!words || !values))) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (n > KF_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "more than 8,192 words in a row");
    if (!row_ok(db->nwords, words, n)) ORBX_FAIL(ORBX_ERR_ARG, "word ids not strictly ascending inside [0, nwords)");
    ORBX_NEED_DEVICE();
    std::lock_guard<std::mutex> lk(db->mu);
    StagedCall sc;
    const size_t o_w = sc.in(words, sizeof(int32_t) * (size_t)n), o_v = sc.in(values, sizeof(double) * (size_t)n);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    if (const int rc = make_room(db, n, sc.stream())) return rc;
    const int s = (int)db->len.size();
    hipLaunchKernelGGL(k_kfdb_append, dim3(std::max(1, (n + MT - 1) / MT)), dim3(MT), 0, sc.stream(), (const int32_t *)sc.d<int32_t>(o_w),
                       (const double *)sc.d<double>(o_v), n, db->d_words, db->d_values, db->d_rows, s, (int)db->used);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipStreamSynchronize(sc.stream()));     // the staging block is the workspace's: the next call may overwrite it
    db->len.push_back(n);
    db->used += (size_t)n;
    db->live++;
    *slot = s;
    return ORBX_OK;
}

int orbm_kfdb_erase(orbm_kfdb *db, int slot)
{
    if (!db) ORBX_FAIL(ORBX_ERR_ARG, "null database");
    std::lock_guard<std::mutex> lk(db->mu);
    if (slot < 0 || (size_t)slot >= db->len.size()) ORBX_FAIL(ORBX_ERR_ARG, "slot out of range");
    if (db->len[slot] < 0) ORBX_FAIL(ORBX_ERR_ARG, "slot erased already");
    ORBX_NEED_DEVICE();
    WorkspaceLease lease;
    const hipStream_t st = lease.w->own_stream();
    if (!st) ORBX_FAIL(ORBX_ERR_HIP, "hipStreamCreate failed");
    const int2 dead = make_int2(0, -1);
    ORBX_HIP(hipMemcpyAsync(db->d_rows + slot, &dead, sizeof(int2), hipMemcpyHostToDevice, st));
    ORBX_HIP(hipStreamSynchronize(st));
    db->len[slot] = -1;
    db->live--;
    return ORBX_OK;
}

int orbm_kfdb_clear(orbm_kfdb *db)
{
    if (!db) ORBX_FAIL(ORBX_ERR_ARG, "null database");
    std::lock_guard<std::mutex> lk(db->mu);
    db->len.clear();                     // slots restart at 0; the slot table's entries are rewritten by add before anything reads them
    db->used = 0;
    db->live = 0;
    return ORBX_OK;
}

int orbm_kfdb_size(const orbm_kfdb *db, int *live, int *slots)
{
    if (!db) ORBX_FAIL(ORBX_ERR_ARG, "null database");
    std::lock_guard<std::mutex> lk(const_cast<orbm_kfdb *>(db)->mu);
    if (live) *live = db->live;
    if (slots) *slots = (int)db->len.size();
    return ORBX_OK;
}

int orbm_debug_kfdb_reallocs(const orbm_kfdb *db)
{
    if (!db) return -1;
    std::lock_guard<std::mutex> lk(const_cast<orbm_kfdb *>(db)->mu);
    return db->reallocs;
}

int orbm_kfdb_query(orbm_kfdb *db, const int32_t *qwords, const double *qvalues, int nq, int32_t *common, int32_t *first, float *score)
{
    if (!db || !common || !first || !score || nq < 0 || (nq && (!qwords || !qvalues))) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (nq > KF_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "more than 8,192 words in the query");
    if (!row_ok(db->nwords, qwords, nq)) ORBX_FAIL(ORBX_ERR_ARG, "word ids not strictly ascending inside [0, nwords)");
    std::lock_guard<std::mutex> lk(db->mu);
    const size_t slots = db->len.size();
    if (db->live == 0 || nq == 0) {      // nothing to launch: needs no device either
        g_last_kfdb_waits.store(0, std::memory_order_relaxed);
        fill_unshared(db, common, first, score);
        return ORBX_OK;
    }
    ORBX_NEED_DEVICE();
    g_last_kfdb_waits.store(0, std::memory_order_relaxed);
    StagedCall sc;
    const size_t o_qw = sc.in(qwords, sizeof(int32_t) * (size_t)nq), o_qv = sc.in(qvalues, sizeof(double) * (size_t)nq);
    const size_t o_c = sc.out(sizeof(int32_t) * slots), o_f = sc.out(sizeof(int32_t) * slots), o_s = sc.out(sizeof(float) * slots);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    if (const int rc = launch_query(db, sc, o_qw, o_qv, nq, nullptr, (int)slots, sc.d<int32_t>(o_c), sc.d<int32_t>(o_f), sc.d<float>(o_s))) return rc;
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    g_last_kfdb_waits.store(sc.waits, std::memory_order_relaxed);
    memcpy(common, sc.r<int32_t>(o_c), sizeof(int32_t) * slots);
    memcpy(first, sc.r<int32_t>(o_f), sizeof(int32_t) * slots);
    memcpy(score, sc.r<float>(o_s), sizeof(float) * slots);
    return ORBX_OK;
}

int orbm_kfdb_score(orbm_kfdb *db, const int32_t *qwords, const double *qvalues, int nq, const int32_t *slots, int n, float *score)
{
    if (!db || nq < 0 || (nq && (!qwords || !qvalues)) || n < 0 || (n && !slots) || !score) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (nq > KF_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "more than 8,192 words in the query");
    if (n > KF_MAXN) ORBX_FAIL(ORBX_ERR_ARG, "more than 8,192 slots in the list");
    if (!row_ok(db->nwords, qwords, nq)) ORBX_FAIL(ORBX_ERR_ARG, "word ids not strictly ascending inside [0, nwords)");
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || (size_t)slots[i] >= db->len.size() || db->len[slots[i]] < 0) ORBX_FAIL(ORBX_ERR_ARG, "dead or out-of-range slot in the list");
    if (n == 0 || nq == 0) {             // nothing to launch: needs no device either
        g_last_kfdb_waits.store(0, std::memory_order_relaxed);
        for (int i = 0; i < n; ++i) score[i] = -0.0f;
        return ORBX_OK;
    }
    ORBX_NEED_DEVICE();
    g_last_kfdb_waits.store(0, std::memory_order_relaxed);
    StagedCall sc;
    const size_t o_qw = sc.in(qwords, sizeof(int32_t) * (size_t)nq), o_qv = sc.in(qvalues, sizeof(double) * (size_t)nq);
    const size_t o_l = sc.in(slots, sizeof(int32_t) * (size_t)n), o_s = sc.out(sizeof(float) * (size_t)n);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    if (const int rc = launch_query(db, sc, o_qw, o_qv, nq, sc.d<int32_t>(o_l), n, nullptr, nullptr, sc.d<float>(o_s))) return rc;
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    g_last_kfdb_waits.store(sc.waits, std::memory_order_relaxed);
    memcpy(score, sc.r<float>(o_s), sizeof(float) * (size_t)n);
    return ORBX_OK;
}

int orbm_debug_kfdb_max_blocks(int blocks)
{
    return g_max_blocks.exchange(blocks > 0 ? blocks : 0, std::memory_order_relaxed);
}

int orbm_debug_last_kfdb_waits(void) { return g_last_kfdb_waits.load(std::memory_order_relaxed); }

} // extern "C"
