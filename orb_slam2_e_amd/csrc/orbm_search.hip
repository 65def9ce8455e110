// orbm_search.hip -- whole ORBmatcher search loops for gfx950, with the reference's
// in-loop bookkeeping and its rotation-consistency check:
//   SearchByProjection(Frame, vector<MapPoint*>, th)         src/ORBmatcher.cc:46-132
//   SearchByProjection(CurrentFrame, LastFrame, th, mono)    :1529-1671
//   SearchByProjection(CurrentFrame, KeyFrame, found, ...)   :1673-1800
//   SearchByProjection(KeyFrame, Scw, points, matched, th)   :491-604
//   SearchForInitialization(F1, F2, prevMatched, ...)        :606-721
//
// These loops are sequential in the reference: a query sees what earlier queries left in
// mvpMapPoints / vMatchedDistance.  Here
//   1. the frame's keypoints are sorted by (grid cell, index): a window's candidates are a
//      few contiguous runs of that array, in Frame::GetFeaturesInArea order (src/Frame.cc:342-395);
//   2. k_win_wave (count, then fill; one wave per query) builds every query's candidate list
//      with its Hamming distances, k_topk keeps each list's 8 best sorted -- the expensive
//      part, fully parallel;
//   3. the resolver commits the queries' choices in the loop's order: as a parallel fixed point (k_resolve_par,
//      k_resolve_init_par, rotation check fused), or, when that does not settle, k_resolve: it walks the queries in order, 64 at
//      a time: every lane selects best / second for its query against the committed state; a lane whose best or second
//      candidate is claimed by an earlier lane of the same batch is a conflict; lanes below the first conflict commit, the
//      rest select again.  A lane's selection can only change when an earlier query claims its best or second candidate, so
//      the committed results are the sequential loop's results.  The decisions are written once and shared by all four
//      resolvers: load_top, select_two (short list, d7 shortcut, whole-list scan), accepts_projection / accepts_initialization;
//      for_each_query walks a fixed-point thread's queries; rotation_bin and three_maxima (orbm_internal.h) are the check's;
//      Queries whose candidate sets cannot meet are independent of each other: the BoW searches hand
//      k_resolve one SEGMENT per vocabulary node (a feature belongs to one node, ORBmatcher.cc:384-456),
//      one workgroup per segment, so the nodes resolve side by side instead of one after the other;
//      whole SEARCHES that share nothing -- SearchByBoW against every candidate keyframe -- run as one call
//      (orbm_frame_search_by_bow_pairs: k_list_fill_pairs, then k_resolve_par_pairs with one fixed-point workgroup per search);
//   4. k_rotation builds the 30-bin rotation histogram, ORBmatcher::ComputeThreeMaxima
//      (:1802-1843) and rejects the matches outside the three main bins.
// The host never waits in the middle of a call (run_sequential over a SeqSearch: seq_layout, seq_stage, seq_lists, seq_resolve,
// seq_collect): the entry buffer is sized per query and the flags that ask for a repeat come back with the results.
// The frames these loops search are made in orbm_frame.hip; the window searches whose queries do not depend on each other, the
// whole-map search among them, are in orbm_window.hip.  The three units share orbm_search_internal.h: a frame comes through
// FrameSrc / FrameView, and SearchBySim3 (below) runs its two directions on the other unit's launch_win_best.
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "common.h"
#include "orbm_internal.h"
#include "orbm_search_internal.h"
#include "orbx_internal.h"
#include "orbx_math.h"

using namespace orbm_detail;

namespace {

enum { ACCEPT_BEST = 0, ACCEPT_RATIO_SAME_LEVEL = 1, ACCEPT_RATIO = 2 };


constexpr int TOPK = 8; // best candidates per query kept sorted for the resolver


// The TOPK entries of a list with the smallest (distance, position) keys, in that
// order -- all the sequential resolver normally needs.  Run by the wave that has just written the list
// (its own stores are visible to it after the workgroup-scope fence).  Lists of up to 256 entries -- a window's usual few tens --
// are read ONCE, four entries per lane, and the rounds run on registers (every round used to re-read the list: eight dependent
// trips to L1 / L2 per query).
// the rounds on registers: every lane holds up to four (key, entry) pairs, keys unique (0xffffffff: none)
__device__ __forceinline__ void wave_topk_regs(unsigned (&key)[4], const unsigned (&en)[4], int lane, unsigned *__restrict__ top_i)
{
#pragma unroll
    for (int t = 0; t < TOPK; ++t) {
        const unsigned g = wave_min_u32(min(min(key[0], key[1]), min(key[2], key[3])));
        if (g == 0xffffffffu) { if (lane == 0) top_i[t] = 0xffffffffu; continue; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (key[r] == g) { top_i[t] = en[r]; key[r] = 0xffffffffu; }     // keys are unique: one lane, one slot
    }
}
__device__ __forceinline__ void wave_topk(const unsigned *__restrict__ ent, int b, int len, int lane, unsigned *__restrict__ top_i)
{
    if (len <= 256) {
        unsigned key[4], en[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = lane + 64 * r;
            en[r] = p < len ? ent[b + p] : 0xffffffffu;
            key[r] = en[r] != 0xffffffffu ? ((en[r] >> 20) << 16) | (unsigned)p : 0xffffffffu;
        }
        wave_topk_regs(key, en, lane, top_i);
        return;
    }
    unsigned prev = 0;
    bool done = false;
    for (int r = 0; r < TOPK; ++r) {
        unsigned g = 0xffffffffu;
        if (!done) {
            unsigned m = 0xffffffffu;
            for (int p = lane; p < len; p += 64) {
                const unsigned en = ent[b + p];
                if (en != 0xffffffffu) {
                    const unsigned key = ((en >> 20) << 16) | (unsigned)p;
                    if (r == 0 || key > prev) m = min(m, key);
                }
            }
            g = wave_min_u32(m);
            done = g == 0xffffffffu;
            prev = g;
        }
        if (lane == 0) top_i[r] = done ? 0xffffffffu : ent[b + (g & 0xffffu)];
    }
}

// One WAVE per query (4 per block).  Frame::GetFeaturesInArea (src/Frame.cc:342-395): the
// cell range of the window in the reference's float arithmetic, then, column by column,
// the keypoints of rows [nMinCellY, nMaxCellY] -- one contiguous run of the (cell, index)
// sorted array -- tested 64 at a time: level range, |dx| < r && |dy| < r, and the stereo
// check of ORBmatcher.cc:91-96.  FILL = 2 (the usual path) writes the survivors of query i into its own region of
// `stride` entries and the region's bounds into lbeg / lend, and raises *overflow if a list does not fit (the host
// then repeats the call on the exact path); FILL = 0 counts the survivors; FILL = 1 writes them in
// that order with their distances: entry = dist << 20 | octave << 16 | sp (0xffffffff for
// a distance that can never be selected).
template <int FILL>
__global__ __launch_bounds__(MT) void k_win_wave(const WinQuery *__restrict__ q, const uint4 *__restrict__ A, int nq,
                                                 const SeqKp *__restrict__ kp, const uint4 *__restrict__ B,
                                                 const int *__restrict__ cell_off, const uint8_t *__restrict__ occ, GridParams gp, int has_uright, int init_dist,
                                                 int *__restrict__ cnt, const int *__restrict__ off, unsigned *__restrict__ ent,
                                                 int stride, int *__restrict__ lbeg, int *__restrict__ lend,
                                                 int *__restrict__ overflow, unsigned *__restrict__ top, int gen)
{
    // (the query index is the same in all lanes: said so, the query record, its cell range and the runs' bounds become scalar loads)
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * (MT / 64) + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (i >= nq) return;
    const int obase = FILL == 2 ? i * stride : (FILL == 1 ? off[i] : 0), ocap = FILL == 2 ? stride : INT_MAX;
    const WinQuery w = q[i];
    int c = 0;
    const int nMinCellX = (int)fmaxf(0.f, floorf((w.u - gp.min_x - w.r) * gp.inv_w));
    const int nMaxCellX = (int)fminf((float)FRAME_GRID_COLS - 1, ceilf((w.u - gp.min_x + w.r) * gp.inv_w));
    const int nMinCellY = (int)fmaxf(0.f, floorf((w.v - gp.min_y - w.r) * gp.inv_h));
    const int nMaxCellY = (int)fminf((float)FRAME_GRID_ROWS - 1, ceilf((w.v - gp.min_y + w.r) * gp.inv_h));
    const bool none = !(w.r >= 0.f) || nMinCellX >= FRAME_GRID_COLS || nMaxCellX < 0 || nMinCellY >= FRAME_GRID_ROWS || nMaxCellY < 0;
    // FILL = 2: the entries a lane produces also stay in its registers (one per 64-candidate step, up to four steps): the short list is
    // then built without reading the list back (a fence and a memory round trip at the end of every wave's life)
    unsigned rkey[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, ren[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    int step = 0;
    if (!none) {
        const bool check_levels = (w.min_level > 0) || (w.max_level >= 0);
        uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
        if (FILL) { a0 = A[2 * i]; a1 = A[2 * i + 1]; }
        unsigned *out = FILL ? ent + obase : nullptr;
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            const int k0 = cell_off[ix * FRAME_GRID_ROWS + nMinCellY], k1 = cell_off[ix * FRAME_GRID_ROWS + nMaxCellY + 1];
            for (int kb = k0; kb < k1; kb += 64) {
                const int k = kb + lane;
                bool ok = k < k1;
                SeqKp p = {0.f, 0.f, 0.f, 0};
                uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0;
                if (ok) {
                    p = kp[k];
                    if (FILL) { b0 = B[2 * k]; b1 = B[2 * k + 1]; }    // with the keypoint, not behind its tests: one memory round trip less per step
                }
                if (occ && ok) ok = occ[k] == 0;   // the slot holds a point from the start (e.g. ORBmatcher.cc:87-89): never a candidate
                if (check_levels) ok = ok && !(p.octave < w.min_level) && !(w.max_level >= 0 && p.octave > w.max_level);
                const float distx = p.x - w.u, disty = p.y - w.v;
                ok = ok && fabsf(distx) < w.r && fabsf(disty) < w.r;
                if (has_uright && p.uright > 0) ok = ok && !(fabsf(w.xr - p.uright) > w.r);
                const unsigned long long bal = __ballot(ok);
                if (FILL && ok && c + __popcll(bal & lt) < ocap) {
                    const int dist = popc256(a0, a1, b0, b1), pos = c + __popcll(bal & lt);
                    const unsigned en = dist < init_dist ? ((unsigned)dist << 20) | ((unsigned)p.octave << 16) | (unsigned)k : 0xffffffffu;
                    out[pos] = en;
                    if (FILL == 2 && en != 0xffffffffu) {
                        const unsigned key = ((unsigned)dist << 16) | (unsigned)pos;
                        if (step == 0) { rkey[0] = key; ren[0] = en; } else if (step == 1) { rkey[1] = key; ren[1] = en; }
                        else if (step == 2) { rkey[2] = key; ren[2] = en; } else if (step == 3) { rkey[3] = key; ren[3] = en; }
                    }
                }
                c += __popcll(bal);
                ++step;
            }
        }
    }
    if (!FILL && lane == 0) cnt[i] = c;
    if (FILL) {
        if (FILL == 2 && lane == 0) {
            lbeg[i] = obase; lend[i] = obase + min(c, ocap);
            if (c > ocap) *overflow = gen;          // this call's generation number: some list did not fit (the word arrives as 0 with the call's staged inputs)
        }
        if (FILL == 2 && step <= 4) {
            wave_topk_regs(rkey, ren, lane, top + (size_t)i * TOPK);
        } else {
            __threadfence_block();
            wave_topk(ent, obase, min(c, ocap), lane, top + (size_t)i * TOPK);
        }
    }
}

// Entries for explicit candidate lists (BoW-node members in member order), one wave per
// query: entry = dist << 20 | candidate index; a distance of 256 can never be selected.  Query i's candidates are
// cand[cbeg[i] .. cbeg[i] + off[i+1] - off[i]): the queries of one node share one copy of the node's member list.
// qmap (queries taken from a resident frame): query i is the feature at sorted position qmap[i] of that frame -- A and qang_src are the
// frame's arrays, and the query's angle is set down in qang_dst[i] for the rotation check.
// list_fill_query is the wave's work, shared by k_list_fill (one search) and k_list_fill_pairs (a batch of searches).  Its pointers
// are not __restrict__ on purpose: k_list_fill's own parameters carry the qualifier, and with it here as well that kernel's register
// allocation moved.
__device__ __forceinline__ void list_fill_query(int i, int lane, const uint4 *A, const uint4 *B, const int *off, const int *cbeg,
                                                const int *cand, unsigned *ent, unsigned *top, const int *qmap,
                                                const float *qang_src, float *qang_dst)
{
    const int qi = qmap ? qmap[i] : i;
    if (qmap && lane == 0) qang_dst[i] = qang_src[qi];
    const uint4 a0 = A[2 * qi], a1 = A[2 * qi + 1];
    const int shift = cbeg[i] - off[i];
    for (int k = off[i] + lane; k < off[i + 1]; k += 64) {
        const int j = cand[k + shift];
        const int dist = popc256(a0, a1, B[2 * j], B[2 * j + 1]);
        ent[k] = dist < 256 ? ((unsigned)dist << 20) | (unsigned)j : 0xffffffffu;
    }
    __threadfence_block();
    wave_topk(ent, off[i], off[i + 1] - off[i], lane, top + (size_t)i * TOPK);
}
__global__ __launch_bounds__(MT) void k_list_fill(const uint4 *__restrict__ A, int nq, const uint4 *__restrict__ B,
                                                  const int *__restrict__ off, const int *__restrict__ cbeg,
                                                  const int *__restrict__ cand, unsigned *__restrict__ ent,
                                                  unsigned *__restrict__ top, const int *__restrict__ qmap,
                                                  const float *__restrict__ qang_src, float *__restrict__ qang_dst)
{
    const int i = blockIdx.x * (MT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nq) return;
    list_fill_query(i, lane, A, B, off, cbeg, cand, ent, top, qmap, qang_src, qang_dst);
}

// One search of a batch of BoW searches over resident frames (orbm_frame_search_by_bow_pairs), as its two kernels read it: the
// two frames' arrays, the search's lists, short lists and angles in the call's workspace, its working copies of the results and
// its rows of the result block in pinned host memory.
struct BowPairDev {
    const uint4 *A, *B;                         // descriptors of frame1 / frame2 by sorted position
    const float *qang_src, *kangle;             // angles of frame1 / frame2 by sorted position
    const int *perm;                            // frame2: keypoint index at sorted position
    const int *qmap, *off, *cbeg, *cand;        // query -> sorted position in frame1; the lists (off[nq + 1] counts from 0)
    unsigned *ent, *top;                        // the search's entries and short lists
    float *qang;                                // [nq] the queries' angles, set down by the list kernel
    int *match_q, *match_kp, *dev_nm;           // device working copies: [nq], [n], [4]
    int *host_q, *host_kp, *host_nm;            // pinned: [nq], [n], [4]
    int nq, ns, n, reserved;                    // queries; positions of frame2 (= its keypoints: addressed by index); keypoints of frame2
};

// k_list_fill for all searches of a batch: blockIdx.y = the search, one wave per query; the grid's first dimension is sized for the
// batch's largest nq, and a wave beyond its search's nq leaves before any work.
__global__ __launch_bounds__(MT) void k_list_fill_pairs(const BowPairDev *__restrict__ recs)
{
    const BowPairDev &p = recs[blockIdx.y];
    const int i = blockIdx.x * (MT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= p.nq) return;
    list_fill_query(i, lane, p.A, p.B, p.off, p.cbeg, p.cand, p.ent, p.top, p.qmap, p.qang_src, p.qang);
}

// Exclusive scan of cnt[0..n) into off[0..n], one block (n is a few thousand).
__global__ __launch_bounds__(MT) void k_scan_counts(const int *__restrict__ cnt, int n, int *__restrict__ off, int *__restrict__ total_out)
{
    __shared__ int part[MT];
    const int tid = threadIdx.x, per = (n + MT - 1) / MT, lo = min(tid * per, n), hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int r = 0;
        for (int i = 0; i < MT; ++i) { const int v = part[i]; part[i] = r; r += v; }
        off[n] = r;
        *total_out = r;
    }
    __syncthreads();
    int r = part[tid];
    for (int i = lo; i < hi; ++i) { off[i] = r; r += cnt[i]; }
}

// ---- The decisions every resolver shares, each written once.
// A list entry is dist << 20 | octave << 16 | sorted position; 0xffffffff = none.
__device__ __forceinline__ int entry_slot(unsigned en) { return (int)(en & 0xffffu); }
__device__ __forceinline__ int entry_level(unsigned en) { return (int)((en >> 16) & 15); }
__device__ __forceinline__ int entry_dist(unsigned en) { return (int)(en >> 20); }

// Query i's short list (the TOPK best entries of its candidate list, sorted) as two 16-byte loads.
__device__ __forceinline__ void load_top(const unsigned *__restrict__ top, int i, unsigned (&tp)[TOPK])
{
    const uint4 t0 = reinterpret_cast<const uint4 *>(top)[2 * (size_t)i], t1 = reinterpret_cast<const uint4 *>(top)[2 * (size_t)i + 1];
    tp[0] = t0.x; tp[1] = t0.y; tp[2] = t0.z; tp[3] = t0.w; tp[4] = t1.x; tp[5] = t1.y; tp[6] = t1.z; tp[7] = t1.w;
}

// The acceptance rule of the projection family and the BoW searches: bestDist <= th, then the ratio test of the form --
// ACCEPT_RATIO_SAME_LEVEL: rejected if best and second sit on the same level and best > ratio * second (:121);
// ACCEPT_RATIO: accepted only if best < ratio * second (:431, :801).  Without a second candidate bestDist2 keeps its
// initial 256 (:79-81).
__device__ __forceinline__ bool accepts_projection(int accept_mode, int best, int second, bool has_second, int l1, int l2, float nnratio, int th)
{
    bool acc = best <= th;
    const int sec = has_second ? second : 256;
    if (accept_mode == ACCEPT_RATIO_SAME_LEVEL && has_second && l1 == l2 && (float)best > nnratio * (float)sec) acc = false;
    if (accept_mode == ACCEPT_RATIO && !((float)best < nnratio * (float)sec)) acc = false;
    return acc;
}
// SearchForInitialization's (:674-676); second = INT_MAX when the best candidate is alone (:637-638).
__device__ __forceinline__ bool accepts_initialization(int best, int second, float nnratio, int th)
{
    return best <= th && (float)best < (float)second * nnratio;
}

// Best and second-best eligible candidate of one query: en1 / en2 = their entries (0xffffffff: none), best / second = their
// distances (INT_MAX: none).  state(sp) = the state of slot sp as this query sees it, open(state, dist) = "the slot is
// eligible"; `want` = 2, or 1 where only the best matters (en2 is then none).
//   1. The first two eligible entries of the short list, which is sorted by (distance, list position) = the reference's
//      strict-'<' first-wins order.  EAGER: the state of all TOPK slots is read at once (one after the other, each behind the
//      test of the one before, they are up to eight dependent LDS round trips); otherwise slot by slot, while still needed.
//   2. The short list ran dry and the list is longer: the whole list is needed only if it can change the DECISION.  Every entry
//      beyond the short list is at least as far as its last one, d7.  With nothing eligible so far, a best beyond d7 must
//      still be <= th.  With one eligible entry, the second best is >= d7 (and <= 256, the reference's initial bestDist2): a best
//      that is rejected by th anyway, or that passes its ratio test against d7 on the same level -- accepts(best, d7) --
//      is decided whatever the second is; `second` is then d7, a lower bound, and en2 none.  Most of a late query's short
//      list is taken by earlier matches, so this case is the common one.
//   3. Otherwise: the two smallest keys dist << 16 | list position among the eligible entries of the whole list.
struct TwoBest { unsigned en1, en2; int best, second; };
template <bool EAGER, typename State, typename Open, typename Accepts>
__device__ __forceinline__ TwoBest select_two(const unsigned (&tp)[TOPK], const unsigned *__restrict__ ent, int b, int e, int want, int th,
                                              State state, Open open, Accepts accepts)
{
    TwoBest s = {0xffffffffu, 0xffffffffu, INT_MAX, INT_MAX};
    int found = 0, st[TOPK];
    if (EAGER) {
#pragma unroll
        for (int r = 0; r < TOPK; ++r) st[r] = state(tp[r] == 0xffffffffu ? 0 : entry_slot(tp[r]));
        if (want < 2) {     // "best only" (wave-uniform): the first open entry of the sorted short list, a select chain
            unsigned en1 = 0xffffffffu;
#pragma unroll
            for (int r = TOPK - 1; r >= 0; --r) en1 = (tp[r] != 0xffffffffu && open(st[r], entry_dist(tp[r]))) ? tp[r] : en1;
            if (en1 != 0xffffffffu || e - b <= TOPK) return {en1, 0xffffffffu, en1 != 0xffffffffu ? entry_dist(en1) : INT_MAX, INT_MAX};
        }
    }
#pragma unroll
    for (int r = 0; r < TOPK; ++r) {
        const unsigned en = tp[r];
        if (en != 0xffffffffu && found < 2) {
            const int dist = entry_dist(en);
            if (open(EAGER ? st[r] : state(entry_slot(en)), dist)) {
                if (found == 0) { s.en1 = en; s.best = dist; } else { s.en2 = en; s.second = dist; }
                ++found;
            }
        }
    }
    bool scan = found < want && e - b > TOPK;
    if (scan) {
        const int d7 = entry_dist(tp[TOPK - 1]);
        if (found == 0) scan = d7 <= th;
        else if (s.best > th || accepts(s.best, d7)) { scan = false; s.second = d7; }
    }
    if (scan) {
        unsigned k1 = 0xffffffffu, k2 = 0xffffffffu;
        for (int k = b; k < e; ++k) {
            const unsigned en = ent[k];
            if (en != 0xffffffffu && open(state(entry_slot(en)), entry_dist(en))) {
                const unsigned key = ((en >> 20) << 16) | (unsigned)(k - b);
                const unsigned hi = max(k1, key);
                k2 = min(k2, hi);
                k1 = min(k1, key);
            }
        }
        s = {0xffffffffu, 0xffffffffu, INT_MAX, INT_MAX};
        if (k1 != 0xffffffffu) { s.en1 = ent[b + (k1 & 0xffffu)]; s.best = (int)(k1 >> 16); }
        if (k2 != 0xffffffffu) { s.en2 = ent[b + (k2 & 0xffffu)]; s.second = (int)(k2 >> 16); }
    }
    if (want < 2) s.en2 = 0xffffffffu;
    return s;
}

// The sequential loop, 64 queries per batch (see the file header).  MODE 0 = projection
// family / BoW: state = blocked[sp] ("the slot holds a point later queries must skip"),
// match_kp[sp] = last query assigned to the slot.  MODE 1 = SearchForInitialization:
// state = vMatchedDistance[sp], vnMatches21[sp], vnMatches12[i].
// A lane selects with select_two: a slot is open while it is not blocked (MODE 0) / while
// its recorded distance is above the query's (MODE 1).
// Conflicts go through a claim table: every accepted lane whose match blocks its slot
// claims it with its lane number (minimum wins); a lane whose best or second slot is
// claimed by a lower lane has to select again after that lane has committed.
// acc_sp[i] = candidate chosen by query i when it was accepted (else -1).
// seg != nullptr: workgroup s resolves the queries [seg[s], seg[s+1]) -- segments whose candidate sets are disjoint
// (BoW nodes) -- on its own copy of the state and writes back only the slots it touched (out_a is preset to -1, the
// match count is added up); seg == nullptr: one workgroup, all queries.
template <int MODE>
__global__ __launch_bounds__(64) void k_resolve(const unsigned *__restrict__ ent, const unsigned *__restrict__ top,
                                                const int *__restrict__ lbeg, const int *__restrict__ lend, int nq_all, int ns, const uint8_t *__restrict__ takes, int th,
                                                float nnratio, int accept_mode, int *__restrict__ acc_sp, int *__restrict__ out_a,
                                                int *__restrict__ nmatches, const int *__restrict__ seg)
{
    const int q_begin = seg ? seg[blockIdx.x] : 0, nq = seg ? seg[blockIdx.x + 1] : nq_all;
    extern __shared__ __align__(16) int sm[];
    int *s_a = sm;            // MODE 0: match_kp[ns]   MODE 1: vMatchedDistance[ns]
    int *s_b = s_a + ns;      // MODE 0: blocked[ns]    MODE 1: vnMatches21[ns]
    int *s_claim = s_b + ns;  // lane that claims the slot in this pass, 64 = none
    int *s_c = s_claim + ns;  // MODE 1: vnMatches12[nq]
    const int lane = threadIdx.x;
    for (int j = lane; j < ns; j += 64) { s_a[j] = MODE == 0 ? -1 : INT_MAX; s_b[j] = MODE == 0 ? 0 : -1; s_claim[j] = 64; }
    if (MODE == 1) for (int j = lane; j < nq; j += 64) s_c[j] = -1;   // MODE 1 never runs in segments
    __syncthreads();
    const bool need2 = MODE == 1 || accept_mode != ACCEPT_BEST;
    int nm = 0;
    // a batch's inputs are fetched while the previous batch is resolved (they do not depend on the state): without
    // this every batch starts with a ~1.5 us round trip to L2 / HBM
    int nb_ = 0, ne_ = 0, ntk = 1;
    unsigned ntp[TOPK];
    auto fetch = [&](int i) {
        nb_ = ne_ = 0; ntk = 1;
#pragma unroll
        for (int k = 0; k < TOPK; ++k) ntp[k] = 0xffffffffu;
        if (i < nq) {
            nb_ = lbeg[i]; ne_ = lend[i];
            load_top(top, i, ntp);
            if (MODE == 0) ntk = takes[i];
        }
    };
    fetch(q_begin + lane);
    const int *s_elig = MODE == 0 ? s_b : s_a;    // what decides whether a slot is open to a query
    for (int i0 = q_begin; i0 < nq; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < nq;
        const int b = nb_, e = ne_;
        unsigned tp[TOPK];
#pragma unroll
        for (int k = 0; k < TOPK; ++k) tp[k] = ntp[k];
        const int tk = ntk;
        fetch(i + 64);
        unsigned long long pending = __ballot(in);
        bool dirty = true;
        TwoBest sel = {0xffffffffu, 0xffffffffu, INT_MAX, INT_MAX};
        while (pending) {
            const bool mine = (pending >> lane) & 1ull;
            if (mine && dirty)
                sel = select_two<true>(tp, ent, b, e, need2 ? 2 : 1, th, [&](int sp) { return s_elig[sp]; },
                                       [&](int st, int dist) { return MODE == 0 ? st == 0 : st > dist; },
                                       [&](int best, int d) {
                                           return MODE == 1 ? accepts_initialization(best, d, nnratio, th)
                                                            : accepts_projection(accept_mode, best, d, true, 0, 0, nnratio, th);
                                       });
            const int sp1 = sel.en1 != 0xffffffffu ? entry_slot(sel.en1) : -1, sp2 = sel.en2 != 0xffffffffu ? entry_slot(sel.en2) : -1;
            const int best = sel.best;
            const bool acc = mine && sp1 >= 0 &&
                             (MODE == 1 ? accepts_initialization(best, sel.second, nnratio, th)
                                        : accepts_projection(accept_mode, best, sel.second, sp2 >= 0, entry_level(sel.en1), entry_level(sel.en2), nnratio, th));
            // claims of this pass
            const bool claims = acc && tk;
            if (claims) atomicMin(&s_claim[sp1], lane);
            __syncthreads();
            const bool conflict = mine && ((sp1 >= 0 && s_claim[sp1] < lane) || (sp2 >= 0 && s_claim[sp2] < lane));
            __syncthreads();
            if (claims) s_claim[sp1] = 64;
            const unsigned long long cm = __ballot(conflict);
            const int lc = cm ? __ffsll((long long)cm) - 1 : 64;
            const bool commit = mine && lane < lc;
            int old = -1;
            if (commit) {
                acc_sp[i] = acc ? sp1 : -1;
                if (acc) {
                    if (MODE == 0) {
                        atomicMax(&s_a[sp1], i);               // the last query assigned to the slot stays
                        if (tk) s_b[sp1] = 1;
                    } else {                                   // accepted candidates of one pass are distinct
                        old = s_b[sp1];
                        if (old >= 0) s_c[old] = -1;           // steal (:678-682)
                        s_c[i] = sp1; s_b[sp1] = i; s_a[sp1] = best;
                    }
                }
            }
            nm += __popcll(__ballot(commit && acc)) - __popcll(__ballot(old >= 0));
            pending &= ~((lc == 64 ? ~0ull : (1ull << lc) - 1ull));
            dirty = conflict;
            __syncthreads();
        }
    }
    __syncthreads();
    if (MODE == 0) {
        for (int j = lane; j < ns; j += 64)                                  // match_kp by sorted position
            if (!seg || s_a[j] >= 0) out_a[j] = s_a[j];
    } else {
        for (int j = lane; j < nq; j += 64) out_a[j] = s_c[j];              // vnMatches12 by sorted position
    }
    if (lane == 0) { if (seg) atomicAdd(nmatches, nm); else *nmatches = nm; }
}

// The projection family's sequential loop as a parallel fixed point, with the rotation check of k_rotation<0> as its tail: ONE
// workgroup of 1024 threads, every query evaluated in every iteration.
//
// In the reference's loop (ORBmatcher.cc:69-130, :1588-1660, ...) query i skips the keypoints an EARLIER query j < i was matched
// to (if j's point blocks the slot: `takes`), and nothing else couples the queries.  Let first[s] be the smallest index of a
// query whose accepted match takes slot s.  Given `first`, query i's selection is a function of it alone: candidates with
// first[s] < i are skipped.  Iterate: all queries select against first_k, their claims give first_{k+1}.  Query 0 never skips
// anything, so it is final after one iteration; once every j < i is final, i is final one iteration later: the iteration reaches
// the sequential loop's result after at most as many iterations as the longest chain "j's match changes what i selects", and a
// state whose claims reproduce themselves is that result (by the same induction).  Real frames have chains of a few queries
// (a window holds a handful of keypoints); the one-wave batch walk of k_resolve took 32 dependent batches for 2,000 queries.
// If the claims still change after RES_MAXIT iterations the kernel says so (*converged = 0) and the host repeats the call on
// k_resolve: the result never depends on how the chains fall.
constexpr int RES_T = 1024, RES_QREG = 2, RES_MAXIT = 48;
// The queries of thread tid of a fixed-point kernel: tid, tid + RES_T, ...  The first RES_QREG of them have a register slot r (their
// short lists, bounds, angles and selections stay in registers from phase to phase); the others (r = -1) go through global
// memory.  f(i, r) is inlined with r a constant, so `r >= 0 ? regs[r] : global[i]` in it costs nothing.
template <typename F>
__device__ __forceinline__ void for_each_query(int tid, int nq, F f)
{
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r)
        if (tid + r * RES_T < nq) f(tid + r * RES_T, r);
    for (int i = tid + RES_QREG * RES_T; i < nq; i += RES_T) f(i, -1);
}
// The kernel's body is resolve_par: ONE workgroup's work on ONE search, whose whole state -- the claim tables, permutation and
// angles in the dynamic LDS `sm` (4 * ns ints), the histogram, the counts and the "changed" word in static LDS -- belongs to the
// workgroup that runs it.  k_resolve_par runs it on a call's search; k_resolve_par_pairs on the search its workgroup index selects.
// ALL_TAKE: every query's match blocks its slot (the BoW searches): there is no `takes` array to read.
template <bool ALL_TAKE>
__device__ __forceinline__ void resolve_par(int *__restrict__ sm, const unsigned *__restrict__ ent, const unsigned *__restrict__ top,
                                            const int *__restrict__ lbeg, const int *__restrict__ lend, int nq, int ns,
                                            const uint8_t *__restrict__ takes, int th, float nnratio, int accept_mode,
                                            const float *__restrict__ qangle, const float *__restrict__ kangle,
                                            const int *__restrict__ perm, int check, int *__restrict__ match_q,
                                            int *__restrict__ match_kp, int n, const int *__restrict__ overflow, int gen,
                                            int *__restrict__ host_q, int *__restrict__ host_kp, int *__restrict__ host_nm,
                                            int *__restrict__ dev_nm)
{
    // dev_nm: the device copy of the count ([0]) and of the "fixed point reached" word ([2]) for work chained behind this kernel
    // (SearchChain), which must not wait for the host to read them.  overflow: k_win_wave<2>'s word in the staged block (nullptr:
    // the lists cannot overflow); it is passed on to the host in host_nm[1].
    // host_*: the call's result block in PINNED HOST memory.  The kernel's last phase writes the results there itself (posted
    // writes over PCIe, each element once): a device-to-host copy behind the kernel cost the call its 5 us plus ~9 us of
    // hand-over between the compute queue and the copy engine.  match_q / match_kp stay the device-side working copies.
    int *f_cur = sm, *f_nxt = sm + ns;     // first[s] of the last / of this iteration (INT_MAX: nobody takes s)
    int *s_perm = sm + 2 * ns;             // what the tail gathers by sorted position sits in LDS before the iterations end:
    float *s_kang = reinterpret_cast<float *>(sm + 3 * ns);   // the kernel is one workgroup of dependent round trips
    __shared__ int s_changed, s_nm, hist[HISTO_LENGTH], keep[3], removed;
    const int tid = threadIdx.x;
    const bool need2 = accept_mode != ACCEPT_BEST;
    // everything that does not depend on the iterations is requested up front: the first RES_QREG queries of a thread keep
    // their short lists (and their angles) in registers, the permutation and the keypoint angles go to LDS, every slot of the
    // result is preset (keypoints outside the grid included: no fill by the host)
    unsigned tpr[RES_QREG][TOPK];
    int br[RES_QREG], er[RES_QREG], tkr[RES_QREG];
    float qar[RES_QREG];
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) {
        const int i = tid + r * RES_T;
        br[r] = er[r] = 0; tkr[r] = 1; qar[r] = 0.f;
#pragma unroll
        for (int k = 0; k < TOPK; ++k) tpr[r][k] = 0xffffffffu;
        if (i < nq) { load_top(top, i, tpr[r]); br[r] = lbeg[i]; er[r] = lend[i]; tkr[r] = ALL_TAKE ? 1 : (int)takes[i]; qar[r] = qangle[i]; }
    }
    for (int j = tid; j < ns; j += RES_T) { f_cur[j] = INT_MAX; f_nxt[j] = INT_MAX; s_perm[j] = perm[j]; s_kang[j] = kangle[j]; }
    for (int j = tid; j < n; j += RES_T) match_kp[j] = -1;
    for (int i = tid + RES_QREG * RES_T; i < nq; i += RES_T) match_q[i] = -2;   // queries beyond the registers keep their last selection here
    if (tid == 0) { s_changed = 0; s_nm = 0; removed = 0; }
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    // query i's accepted candidate against `first` (or -1): the selection of k_resolve<0>, a slot is open while first[sp] >= i
    auto select = [&](int i, const unsigned (&tp)[TOPK], int b, int e, const int *first) -> int {
        const TwoBest s = select_two<true>(tp, ent, b, e, need2 ? 2 : 1, th, [&](int sp) { return first[sp]; },
                                           [&](int st, int) { return st >= i; },
                                           [&](int best, int d) { return accepts_projection(accept_mode, best, d, true, 0, 0, nnratio, th); });
        const bool acc = s.en1 != 0xffffffffu && accepts_projection(accept_mode, s.best, s.second, s.en2 != 0xffffffffu, entry_level(s.en1),
                                                                    entry_level(s.en2), nnratio, th);
        return acc ? entry_slot(s.en1) : -1;
    };
    __syncthreads();
    int selr[RES_QREG];
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) selr[r] = -2;
    bool done = false;
    int it = 0;
    for (; it < RES_MAXIT; ++it) {
        bool changed = false;
        for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
            unsigned tpg[TOPK];
            if (r < 0) load_top(top, i, tpg);
            const int sel = r >= 0 ? select(i, tpr[r], br[r], er[r], f_cur) : select(i, tpg, lbeg[i], lend[i], f_cur);
            const int prev = r >= 0 ? selr[r] : match_q[i], tk = r >= 0 ? tkr[r] : (ALL_TAKE ? 1 : (int)takes[i]);
            const int claim = sel >= 0 && tk ? sel : -1, was = prev >= 0 && tk ? prev : -1;
            changed |= claim != was || prev == -2;
            if (r >= 0) selr[r] = sel; else match_q[i] = sel;
            if (claim >= 0) atomicMin(&f_nxt[claim], i);
        });
        if (changed) s_changed = 1;
        __syncthreads();
        done = s_changed == 0;
        __syncthreads();
        if (done) break;
        if (tid == 0) s_changed = 0;
        for (int j = tid; j < ns; j += RES_T) f_cur[j] = INT_MAX;     // becomes the next iteration's claim table
        int *t = f_cur; f_cur = f_nxt; f_nxt = t;
        __syncthreads();
    }
    if (tid == 0) host_nm[1] = overflow ? *overflow : 0;      // "a list outgrew its region" as k_win_wave left it
    if (!done) {            // chains longer than RES_MAXIT: the host repeats the call on the sequential kernel
        if (tid == 0) { host_nm[2] = 0; dev_nm[2] = 0; }
        return;
    }
    if (tid == 0) { host_nm[2] = gen; host_nm[3] = it + 1; dev_nm[2] = gen; }   // reached the fixed point (+ the number of iterations it took)
    // ---- tail: match_kp = the LAST accepted query of a slot (:125), the rotation histogram, ComputeThreeMaxima, rejection
    int *s_a = f_nxt;       // (f_nxt holds this iteration's claims = f_cur's content: no longer needed)
    for (int j = tid; j < ns; j += RES_T) s_a[j] = -1;
    __syncthreads();
    auto bin_of = [&](float qa, int sp) { return rotation_bin(qa - s_kang[sp]); };
    int binr[RES_QREG], nacc = 0;     // (the register queries keep their bin for the rejection pass)
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) binr[r] = -1;
    for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
        const int sel = r >= 0 ? selr[r] : match_q[i];
        if (sel < 0) return;
        atomicMax(&s_a[sel], i);
        ++nacc;
        if (check) {
            const int bin = bin_of(r >= 0 ? qar[r] : qangle[i], sel);
            if (r >= 0) binr[r] = bin;
            atomicAdd(&hist[bin], 1);
        }
    });
    if (nacc) atomicAdd(&s_nm, nacc);
    __syncthreads();
    if (tid == 0) three_maxima(hist, keep);
    for (int j = tid; j < ns; j += RES_T)
        if (s_a[j] >= 0) match_kp[s_perm[j]] = s_a[j];        // (the other slots keep their preset -1)
    __syncthreads();
    for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
        const int sp = r >= 0 ? selr[r] : match_q[i];
        const int bin = r >= 0 ? binr[r] : (check && sp >= 0 ? bin_of(qangle[i], sp) : -1);
        if (check && sp >= 0 && bin != keep[0] && bin != keep[1] && bin != keep[2]) { match_kp[s_perm[sp]] = -2; atomicAdd(&removed, 1); }
        host_q[i] = sp >= 0 ? s_perm[sp] : -1;
    });
    __syncthreads();
    for (int j = tid; j < n; j += RES_T) host_kp[j] = match_kp[j];
    if (tid == 0) { host_nm[0] = s_nm - removed; dev_nm[0] = s_nm - removed; }
}
__global__ __launch_bounds__(RES_T) void k_resolve_par(const unsigned *__restrict__ ent, const unsigned *__restrict__ top,
                                                       const int *__restrict__ lbeg, const int *__restrict__ lend, int nq, int ns,
                                                       const uint8_t *__restrict__ takes, int th, float nnratio, int accept_mode,
                                                       const float *__restrict__ qangle, const float *__restrict__ kangle,
                                                       const int *__restrict__ perm, int check, int *__restrict__ match_q,
                                                       int *__restrict__ match_kp, int n, const int *__restrict__ overflow, int gen,
                                                       int *__restrict__ host_q, int *__restrict__ host_kp, int *__restrict__ host_nm,
                                                       int *__restrict__ dev_nm)
{
    extern __shared__ __align__(16) int sm[];
    resolve_par<false>(sm, ent, top, lbeg, lend, nq, ns, takes, th, nnratio, accept_mode, qangle, kangle, perm, check, match_q, match_kp, n,
                       overflow, gen, host_q, host_kp, host_nm, dev_nm);
}
// One 1024-thread workgroup PER SEARCH of a batch of BoW searches: workgroup b resolves the search of record b, on its own LDS
// (the launch asks for the dynamic LDS of the batch's largest ns; a workgroup lays out its own ns).  Workgroups never wait for
// each other; one whose chains exceed RES_MAXIT says so in ITS result row and touches no other.
__global__ __launch_bounds__(RES_T) void k_resolve_par_pairs(const BowPairDev *__restrict__ recs, int th, float nnratio, int check, int gen)
{
    extern __shared__ __align__(16) int sm[];
    const BowPairDev &p = recs[blockIdx.x];
    resolve_par<true>(sm, p.ent, p.top, p.off, p.off + 1, p.nq, p.ns, nullptr, th, nnratio, ACCEPT_RATIO, p.qang, p.kangle, p.perm, check,
                      p.match_q, p.match_kp, p.n, nullptr, gen, p.host_q, p.host_kp, p.host_nm, p.dev_nm);
}

// SearchForInitialization's loop (ORBmatcher.cc:626-696) as a parallel fixed point.  What couples its queries is
// vMatchedDistance: query i leaves a candidate s out of BOTH its best and its second best when an EARLIER query that accepted s
// did so at a distance <= dist(i, s) (:645-646); a later acceptor takes the keypoint from the earlier one (:678-682), and since
// it can only accept s at a distance below the recorded one, vMatchedDistance[s] as query i sees it is M_i(s) = min { d_j : j < i,
// query j accepted s }.  Given every query's accepted (slot, distance), every query's selection is a function of those alone;
// iterate from "nobody has accepted anything": query 0 is final after one iteration, and once all j < i are final so is i one
// iteration later -- a state that reproduces itself is the sequential loop's (the induction of k_resolve_par).  The acceptors
// of a slot sit in a per-slot list of C entries (query << 9 | distance), rebuilt every iteration; a slot with more acceptors
// than that, or chains longer than RES_MAXIT, end the kernel unconverged and the host repeats the call on k_resolve<1>.
// Tail = k_rotation<1>: the match of a slot is its LAST acceptor (the steals), the histogram counts every acceptor, stolen
// or not (:684-693: rotHist keeps them), only standing matches are removed (:704-708).
__global__ __launch_bounds__(RES_T) void k_resolve_init_par(const unsigned *__restrict__ ent, const unsigned *__restrict__ top,
                                                            const int *__restrict__ lbeg, const int *__restrict__ lend, int nq, int ns,
                                                            int C, int th, float nnratio, const float *__restrict__ qangle,
                                                            const float *__restrict__ kangle, const int *__restrict__ perm, int check,
                                                            unsigned *__restrict__ sel_g, const int *__restrict__ overflow, int gen,
                                                            int *__restrict__ host_q, int *__restrict__ host_nm)
{
    extern __shared__ __align__(16) int sm[];
    int *s_cnt = sm, *s_lst = sm + ns;                 // acceptors of slot s: s_lst[s * C .. + min(s_cnt[s], C))
    int *s_perm = sm + (size_t)ns * (C + 1);
    float *s_kang = reinterpret_cast<float *>(sm + (size_t)ns * (C + 2));
    __shared__ int s_changed, s_over, s_nm, hist[HISTO_LENGTH], keep[3], removed;
    const int tid = threadIdx.x;
    unsigned tpr[RES_QREG][TOPK];
    int br[RES_QREG], er[RES_QREG];
    float qar[RES_QREG];
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) {
        const int i = tid + r * RES_T;
        br[r] = er[r] = 0; qar[r] = 0.f;
#pragma unroll
        for (int k = 0; k < TOPK; ++k) tpr[r][k] = 0xffffffffu;
        if (i < nq) { load_top(top, i, tpr[r]); br[r] = lbeg[i]; er[r] = lend[i]; qar[r] = qangle[i]; }
    }
    for (int j = tid; j < ns; j += RES_T) { s_cnt[j] = 0; s_perm[j] = perm[j]; s_kang[j] = kangle[j]; }
    for (int i = tid + RES_QREG * RES_T; i < nq; i += RES_T) sel_g[i] = 0xfffffffeu;   // queries beyond the registers keep their selection here
    if (tid == 0) { s_changed = 0; s_over = 0; s_nm = 0; removed = 0; }
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    // vMatchedDistance[sp] as query i sees it
    auto matched_before = [&](int sp, int i) -> int {
        const int c = min(s_cnt[sp], C);
        int m = INT_MAX;
        for (int k = 0; k < c; ++k) {
            const int v = s_lst[sp * C + k];
            if ((v >> 9) < i) m = min(m, v & 511);
        }
        return m;
    };
    // query i's accepted entry (dist << 20 | octave << 16 | sp) or 0xffffffff: the selection of k_resolve<1>
    auto select = [&](int i, const unsigned (&tp)[TOPK], int b, int e) -> unsigned {
        const TwoBest s = select_two<false>(tp, ent, b, e, 2, th, [&](int sp) { return matched_before(sp, i); },
                                            [&](int st, int dist) { return st > dist; },
                                            [&](int best, int d) { return accepts_initialization(best, d, nnratio, th); });
        return s.en1 != 0xffffffffu && accepts_initialization(s.best, s.second, nnratio, th) ? s.en1 : 0xffffffffu;
    };
    auto claim = [&](int i, unsigned en) {
        if (en == 0xffffffffu) return;
        const int sp = (int)(en & 0xffffu), k = atomicAdd(&s_cnt[sp], 1);
        if (k < C) s_lst[sp * C + k] = (i << 9) | (int)(en >> 20); else s_over = 1;
    };
    __syncthreads();
    unsigned selr[RES_QREG];
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) selr[r] = 0xfffffffeu;
    bool done = false;
    int it = 0;
    for (; it < RES_MAXIT; ++it) {
        bool changed = false;
        for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
            unsigned tpg[TOPK];
            if (r < 0) load_top(top, i, tpg);
            const unsigned en = r >= 0 ? select(i, tpr[r], br[r], er[r]) : select(i, tpg, lbeg[i], lend[i]);
            changed |= en != (r >= 0 ? selr[r] : sel_g[i]);
            if (r >= 0) selr[r] = en; else sel_g[i] = en;
        });
        if (changed) s_changed = 1;
        __syncthreads();
        done = s_changed == 0;
        __syncthreads();
        if (done) break;
        if (tid == 0) s_changed = 0;
        for (int j = tid; j < ns; j += RES_T) s_cnt[j] = 0;
        __syncthreads();
        for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) { claim(i, r >= 0 ? selr[r] : sel_g[i]); });
        __syncthreads();
        if (s_over) break;
    }
    if (tid == 0) host_nm[1] = overflow ? *overflow : 0;      // "a list outgrew its region" as k_win_wave left it
    if (!done) {            // a crowded slot or chains longer than RES_MAXIT: the host repeats the call on the sequential kernel
        if (tid == 0) host_nm[2] = 0;
        return;
    }
    if (tid == 0) { host_nm[2] = gen; host_nm[3] = it + 1; }
    // ---- tail: the standing match of a slot is its last acceptor; rotation histogram over all acceptors; rejection
    int *s_last = s_cnt;
    for (int j = tid; j < ns; j += RES_T) s_last[j] = -1;
    __syncthreads();
    auto bin_of = [&](float qa, int sp) { return rotation_bin(qa - s_kang[sp]); };
    int binr[RES_QREG];
#pragma unroll
    for (int r = 0; r < RES_QREG; ++r) binr[r] = -1;
    for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
        const unsigned en = r >= 0 ? selr[r] : sel_g[i];
        if (en == 0xffffffffu) return;
        atomicMax(&s_last[entry_slot(en)], i);
        if (check) {
            const int bin = bin_of(r >= 0 ? qar[r] : qangle[i], entry_slot(en));
            if (r >= 0) binr[r] = bin;
            atomicAdd(&hist[bin], 1);
        }
    });
    __syncthreads();
    if (tid == 0) three_maxima(hist, keep);
    int nst = 0;
    for (int j = tid; j < ns; j += RES_T) nst += s_last[j] >= 0;     // nmatches before the rotation check = slots that hold a match
    if (nst) atomicAdd(&s_nm, nst);
    __syncthreads();
    for_each_query(tid, nq, [&](int i, int r) __attribute__((always_inline)) {
        const unsigned en = r >= 0 ? selr[r] : sel_g[i];
        int out = -1;
        if (en != 0xffffffffu && s_last[entry_slot(en)] == i) {      // still standing
            const int bin = r >= 0 ? binr[r] : (check ? bin_of(qangle[i], entry_slot(en)) : -1);
            out = s_perm[entry_slot(en)];
            if (check && bin != keep[0] && bin != keep[1] && bin != keep[2]) { out = -1; atomicAdd(&removed, 1); }
        }
        host_q[i] = out;
    });
    __syncthreads();
    if (tid == 0) host_nm[0] = s_nm - removed;
}

// The upload of a call's staged inputs (orbx::stage_in: pinned host memory read by the compute queue) folded into the call's first
// kernel: blocks [0, nblocks) of the launch copy 16 bytes per thread, the others do the kernel's own work and read THEIR inputs --
// which nothing else needs on the device -- straight from the pinned block.  One launch less per call.
struct StageJob { const uint4 *src; uint4 *dst; size_t n16; int nblocks; };
__device__ __forceinline__ bool stage_block(const StageJob &job)
{
    if ((int)blockIdx.x >= job.nblocks) return false;
    const size_t i = (size_t)blockIdx.x * MT + threadIdx.x;
    if (i < job.n16) job.dst[i] = job.src[i];
    return true;
}
inline StageJob stage_job(void *dev, const void *pin, size_t bytes)
{
    return {static_cast<const uint4 *>(pin), static_cast<uint4 *>(dev), bytes / 16, (int)((bytes / 16 + MT - 1) / MT)};
}

// Batch projection of map points into a Frame / KeyFrame: one thread per point runs project_point (orbm_search_internal.h, where
// the modes and the restated cv::Mat arithmetic are described).
__global__ __launch_bounds__(MT) void k_project_points(const uint8_t *__restrict__ valid, const float *__restrict__ pos, const float *__restrict__ nrm,
                                                       const float *__restrict__ mind, const float *__restrict__ maxd, int m,
                                                       ProjectCam cam, const float *__restrict__ scale,
                                                       orbm_projected_point *__restrict__ out, WinQuery *__restrict__ q, StageJob job)
{
    if (stage_block(job)) return;
    const int i = (blockIdx.x - job.nblocks) * MT + threadIdx.x;
    if (i >= m) return;
    orbm_projected_point o;
    WinQuery w;
    project_point(i, valid, pos, nrm, mind, maxd, cam, scale, o, w);
    out[i] = o;
    if (q) q[i] = w;
}

// Rotation histogram + ComputeThreeMaxima (:1802-1843) + rejection, and the translation of
// sorted positions back to keypoint indices.  One block.
// MODE 0: match_kp[perm[sp]] = query (or -1 untouched / -2 cleared), match_q[i] = keypoint.
// MODE 1: match12[i] = keypoint or -1.
template <int MODE>
__global__ __launch_bounds__(MT) void k_rotation(const int *__restrict__ acc_sp, const int *__restrict__ state, int nq, int ns,
                                                 const float *__restrict__ qangle, const float *__restrict__ kangle,
                                                 const int *__restrict__ perm, int check, int *__restrict__ match_q,
                                                 int *__restrict__ match_kp, int *__restrict__ nmatches, const int *__restrict__ overflow)
{
    // nmatches: the result block's four words; [1] takes k_win_wave<2>'s overflow word from the staged block (nullptr: the lists cannot
    // overflow), so that it reaches the host with the results
    __shared__ int hist[HISTO_LENGTH], keep[3], removed;
    const int tid = threadIdx.x;
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) removed = 0;
    __syncthreads();
    auto bin_of = [&](int i, int sp) { return rotation_bin(qangle[i] - kangle[sp]); };
    // the first RPT * MT queries keep (candidate, bin) in registers between the two passes: one dependent gather chain
    // instead of two (the kernel is one block of pure latency)
    constexpr int RPT = 12;
    int spc[RPT], binc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int i = tid + r * MT;
        spc[r] = i < nq ? acc_sp[i] : -1;
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        binc[r] = -1;
        if (check && spc[r] >= 0) { binc[r] = bin_of(tid + r * MT, spc[r]); atomicAdd(&hist[binc[r]], 1); }
    }
    if (check)
        for (int i = tid + RPT * MT; i < nq; i += MT) {
            const int sp = acc_sp[i];
            if (sp >= 0) atomicAdd(&hist[bin_of(i, sp)], 1);
        }
    __syncthreads();
    if (tid == 0) three_maxima(hist, keep);
    if (MODE == 0) for (int j = tid; j < ns; j += MT) match_kp[perm[j]] = state[j];
    __syncthreads();
    auto finish = [&](int i, int sp, int bin) {
        int out = MODE == 0 ? (sp >= 0 ? perm[sp] : -1) : (state[i] >= 0 ? perm[state[i]] : -1);
        if (check && sp >= 0 && bin != keep[0] && bin != keep[1] && bin != keep[2]) {
            if (MODE == 0) { match_kp[perm[sp]] = -2; atomicAdd(&removed, 1); }   // every entry of the bin: slot cleared, nmatches--
            else if (state[i] >= 0) { out = -1; atomicAdd(&removed, 1); }         // only matches still standing (:704-708)
        }
        match_q[i] = out;
    };
#pragma unroll
    for (int r = 0; r < RPT; ++r)
        if (tid + r * MT < nq) finish(tid + r * MT, spc[r], binc[r]);
    for (int i = tid + RPT * MT; i < nq; i += MT) {
        const int sp = acc_sp[i];
        finish(i, sp, check && sp >= 0 ? bin_of(i, sp) : -1);
    }
    __syncthreads();
    if (tid == 0) { nmatches[0] -= removed; nmatches[1] = overflow ? *overflow : 0; }
}

// The projection prefixes of the remaining SearchByProjection forms and of SearchBySim3, one thread per list entry, in the
// reference's float / double order op by op (cv::Mat arithmetic as project_point restates it, orbm_search_internal.h):
//   FORM_LAST   SearchByProjection(CurrentFrame, LastFrame, th, bMono)            src/ORBmatcher.cc:1557-1591
//   FORM_KF     SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) :1702-1735  (no depth test, as the reference)
//   FORM_SIM3   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)             :518-563    (pose = the decomposed Scw)
//   FORM_PAIR   one direction of SearchBySim3                                     :1360-1396 / :1442-1478 (two transforms)
// Output: the GetFeaturesInArea query of every entry (r < 0: the entry is skipped before the search).  project_form_entry is
// entry i of a list under `cam` (FormCam: orbm_search_internal.h); k_project_form runs one list, k_project_pair_jobs the FORM_PAIR
// lists of a batch of SearchBySim3 attempts (orbm_refine_sim3.hip).
__device__ __forceinline__ WinQuery project_form_entry(int i, const uint8_t *__restrict__ valid, const float *__restrict__ pos,
                                                       const float *__restrict__ nrm, const float *__restrict__ mind,
                                                       const float *__restrict__ maxd, const int *__restrict__ octave, const FormCam &cam,
                                                       const float *__restrict__ scale)
{
    WinQuery w = {0.f, 0.f, -1.f, 0.f, 0, -1}; // r < 0: no candidates
    if (valid[i]) {
        const float P0 = pos[3 * i], P1 = pos[3 * i + 1], P2 = pos[3 * i + 2];
        float X = gemm_row(cam.R, 0, P0, P1, P2, cam.t[0]), Y = gemm_row(cam.R, 1, P0, P1, P2, cam.t[1]),
              Z = gemm_row(cam.R, 2, P0, P1, P2, cam.t[2]);
        if (cam.form == FORM_LAST) {
            const float invzc = (float)(1.0 / (double)Z);                          // :1565
            bool ok = !(invzc < 0);
            const float u = cam.fx * X * invzc + cam.cx, v = cam.fy * Y * invzc + cam.cy;
            ok = ok && !(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y);
            if (ok) {
                const int oct = octave[i];
                w.u = u; w.v = v; w.r = cam.th * scale[oct]; w.xr = u - cam.mbf * invzc;
                w.min_level = cam.forward ? oct : (cam.backward ? 0 : oct - 1);     // :1586-1591
                w.max_level = cam.forward ? -1 : (cam.backward ? oct : oct + 1);
            }
        } else if (cam.form == FORM_KF) {
            const float invzc = (float)(1.0 / (double)Z);                          // :1711
            const float u = cam.fx * X * invzc + cam.cx, v = cam.fy * Y * invzc + cam.cy;
            bool ok = !(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y);
            const float PO0 = P0 - cam.Ow[0], PO1 = P1 - cam.Ow[1], PO2 = P2 - cam.Ow[2];
            const float dist3D = (float)sqrt((double)PO0 * (double)PO0 + (double)PO1 * (double)PO1 + (double)PO2 * (double)PO2);
            const float maxDistance = 1.2f * maxd[i], minDistance = 0.8f * mind[i];
            ok = ok && !(dist3D < minDistance || dist3D > maxDistance);
            if (ok) {
                const float ratio = maxd[i] / dist3D;
                int level = orbx_f2i_x86(ceilf(orbx_logf_glibc_f32(ratio) / cam.log_scale));
                if (level < 0) level = 0; else if (level >= cam.nlevels) level = cam.nlevels - 1;
                w.u = u; w.v = v; w.r = cam.th * scale[level]; w.min_level = level - 1; w.max_level = level + 1;
            }
        } else {
            if (cam.form == FORM_PAIR) {     // p3Dc2 = sR21 * (R1w * p3Dw + t1w) + t21
                const float a0 = X, a1 = Y, a2 = Z;
                X = gemm_row(cam.R2, 0, a0, a1, a2, cam.t2[0]); Y = gemm_row(cam.R2, 1, a0, a1, a2, cam.t2[1]);
                Z = gemm_row(cam.R2, 2, a0, a1, a2, cam.t2[2]);
            }
            bool ok = !(Z < 0.0f);
            const float invz = cam.form == FORM_SIM3 ? 1 / Z : (float)(1.0 / (double)Z);      // :531 / :1367
            const float x = X * invz, y = Y * invz;
            const float u = cam.fx * x + cam.cx, v = cam.fy * y + cam.cy;
            ok = ok && (u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y);  // KeyFrame::IsInImage
            const float maxDistance = 1.2f * maxd[i], minDistance = 0.8f * mind[i];
            float dist;
            if (cam.form == FORM_SIM3) {
                const float PO0 = P0 - cam.Ow[0], PO1 = P1 - cam.Ow[1], PO2 = P2 - cam.Ow[2];
                dist = (float)sqrt((double)PO0 * (double)PO0 + (double)PO1 * (double)PO1 + (double)PO2 * (double)PO2);
                ok = ok && !(dist < minDistance || dist > maxDistance);
                const double dot = (double)PO0 * (double)nrm[3 * i] + (double)PO1 * (double)nrm[3 * i + 1] + (double)PO2 * (double)nrm[3 * i + 2];
                ok = ok && !(dot < 0.5 * (double)dist);
            } else {
                dist = (float)sqrt((double)X * (double)X + (double)Y * (double)Y + (double)Z * (double)Z);   // cv::norm(p3Dc2)
                ok = ok && !(dist < minDistance || dist > maxDistance);
            }
            if (ok) {
                const float ratio = maxd[i] / dist;
                int level = orbx_f2i_x86(ceilf(orbx_logf_glibc_f32(ratio) / cam.log_scale));
                if (level < 0) level = 0; else if (level >= cam.nlevels) level = cam.nlevels - 1;
                w.u = u; w.v = v; w.r = cam.th * scale[level]; w.min_level = level - 1; w.max_level = level;
            }
        }
    }
    return w;
}

__global__ __launch_bounds__(MT) void k_project_form(const uint8_t *__restrict__ valid, const float *__restrict__ pos,
                                                     const float *__restrict__ nrm, const float *__restrict__ mind,
                                                     const float *__restrict__ maxd, const int *__restrict__ octave, int m, FormCam cam,
                                                     const float *__restrict__ scale, WinQuery *__restrict__ q, StageJob job)
{
    if (stage_block(job)) return;
    const int i = (blockIdx.x - job.nblocks) * MT + threadIdx.x;
    if (i >= m) return;
    q[i] = project_form_entry(i, valid, pos, nrm, mind, maxd, octave, cam, scale);
}

// SearchBySim3's two projection passes for every (attempt, direction) of a batch: job blockIdx.y, entry by blockIdx.x
__global__ __launch_bounds__(MT) void k_project_pair_jobs(const PairSearchJob *__restrict__ jobs, char *__restrict__ ws, const float *__restrict__ scale)
{
    const PairSearchJob &J = jobs[blockIdx.y];
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= J.nq) return;
    reinterpret_cast<WinQuery *>(ws + J.o_q)[i] =
        project_form_entry(i, reinterpret_cast<const uint8_t *>(ws + J.o_valid), reinterpret_cast<const float *>(ws + J.o_pos), nullptr,
                           reinterpret_cast<const float *>(ws + J.o_min), reinterpret_cast<const float *>(ws + J.o_max), nullptr, J.cam, scale);
}

// SearchBySim3's acceptance and agreement check (src/ORBmatcher.cc:1426-1429, :1505-1507, :1509-1524) over the two window searches.
__global__ __launch_bounds__(MT) void k_sim3_agree(const int *__restrict__ best1, const int *__restrict__ idx1, int n1,
                                                   const int *__restrict__ best2, const int *__restrict__ idx2, int n2, int th_high,
                                                   int *__restrict__ vn1, int *__restrict__ vn2, int *__restrict__ m12, int *__restrict__ nfound)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i < n2) vn2[i] = sim3_accepted(best2[i], idx2[i], th_high);
    bool found = false;
    if (i < n1) {
        const int a = sim3_accepted(best1[i], idx1[i], th_high);
        vn1[i] = a;
        found = sim3_agreed(i, a, best2, idx2, n2, th_high);
        m12[i] = found ? a : -1;
    }
    const unsigned long long b = __ballot(found);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(nfound, __popcll(b));
}

std::atomic<int> g_last_search_waits{0};  // host waits of the last whole-loop search that launched (orbm_debug_last_search_waits)
std::atomic<int> g_last_iterations{0};    // iterations of the last k_resolve_par (-1: it gave up and k_resolve ran)
std::atomic<int> g_force_sequential{0};   // orbm_debug_force_sequential_resolver: tests run both resolvers
std::atomic<int> g_last_bow_pairs_waits{0};   // host waits of the last orbm_frame_search_by_bow_pairs

// A list of map points as the whole-function searches take it (orbm_points), staged with a call, and the prefix kernel that
// turns it into window queries on the device.
struct PointsPrefix {
    const orbm_points *pts = nullptr;
    FormCam cam;
    const float *scale = nullptr;
    bool frustum = false;        // Frame::isInFrustum + the window of SearchByProjection(Frame&, vector<MapPoint*>&, th): k_project_points, mode 0
    ProjectCam pcam;
    orbm_projected_point *proj_host = nullptr;   // optional: the projections back to the caller
    size_t o_proj = 0;
    void carve_scratch(Workspace &w) { if (frustum) o_proj = w.carve(sizeof(orbm_projected_point) * (size_t)(pts->n ? pts->n : 1)); }
    size_t o_valid = 0, o_pos = 0, o_nrm = 0, o_min = 0, o_max = 0, o_oct = 0, o_sc = 0;
    void carve(Workspace &w)
    {
        const size_t m = pts->n ? (size_t)pts->n : 1;
        o_valid = w.carve(m); o_pos = w.carve(sizeof(float) * 3 * m);
        o_nrm = w.carve(pts->normal ? sizeof(float) * 3 * m : 1);
        o_min = w.carve(pts->min_distance ? sizeof(float) * m : 1); o_max = w.carve(pts->max_distance ? sizeof(float) * m : 1);
        o_oct = w.carve(pts->octave ? sizeof(int) * m : 1);
        o_sc = w.carve(sizeof(float) * cam.nlevels);
    }
    void fill(Workspace &w) const
    {
        const size_t m = (size_t)pts->n;
        memcpy(w.h<char>(o_valid), pts->valid, m);
        memcpy(w.h<char>(o_pos), pts->pos, sizeof(float) * 3 * m);
        if (pts->normal) memcpy(w.h<char>(o_nrm), pts->normal, sizeof(float) * 3 * m);
        if (pts->min_distance) memcpy(w.h<char>(o_min), pts->min_distance, sizeof(float) * m);
        if (pts->max_distance) memcpy(w.h<char>(o_max), pts->max_distance, sizeof(float) * m);
        if (pts->octave) memcpy(w.h<char>(o_oct), pts->octave, sizeof(int) * m);
        memcpy(w.h<char>(o_sc), scale, sizeof(float) * cam.nlevels);
    }
    // the prefix's inputs are read where the host staged them (pinned memory); `job` = the call's upload, done by the same launch
    void launch(const Workspace &w, WinQuery *dq, hipStream_t st, StageJob job = StageJob{nullptr, nullptr, 0, 0}) const
    {
        const int nb = (pts->n + MT - 1) / MT + job.nblocks;
        if (!nb) return;
        if (frustum) {
            hipLaunchKernelGGL(k_project_points, dim3(nb), dim3(MT), 0, st, (const uint8_t *)w.h<uint8_t>(o_valid),
                               (const float *)w.h<float>(o_pos), (const float *)w.h<float>(o_nrm), (const float *)w.h<float>(o_min),
                               (const float *)w.h<float>(o_max), pts->n, pcam, (const float *)w.h<float>(o_sc), w.d<orbm_projected_point>(o_proj), dq, job);
            return;
        }
        hipLaunchKernelGGL(k_project_form, dim3(nb), dim3(MT), 0, st, (const uint8_t *)w.h<uint8_t>(o_valid),
                           (const float *)w.h<float>(o_pos), (const float *)w.h<float>(o_nrm), (const float *)w.h<float>(o_min),
                           (const float *)w.h<float>(o_max), (const int *)w.h<int>(o_oct), pts->n, cam, (const float *)w.h<float>(o_sc), dq, job);
    }
};

// ---- The shared driver of the whole-loop searches.  One search as it takes it; a caller sets the fields it uses by name.
struct SeqSearch {
    // The candidates come from ONE of: windows from the host (`queries`), windows made on the device by `prefix` (queries_out, if
    // given, receives them), or explicit candidate lists (BoW-node members).
    const WinQuery *queries = nullptr;
    PointsPrefix *prefix = nullptr;
    struct Lists {      // query i's candidates are idx[beg[i] .. beg[i] + off[i + 1] - off[i]): the queries of a node share one copy
        const int32_t *off = nullptr, *beg = nullptr, *idx = nullptr, *seg = nullptr;
        int n = 0, nseg = 0;    // entries of idx; optional segments: queries [seg[s], seg[s + 1]) share no candidate with the others
    } lists;
    // The queries' descriptors and angles come from ONE of: host arrays (angle = nullptr: all 0), or (candidate lists only) a
    // resident frame: query i is the feature at sorted position pos[i] of `frame`.
    struct Features { const uint8_t *desc = nullptr; const float *angle = nullptr; const orbm_frame *frame = nullptr; const int32_t *pos = nullptr; } q;
    const uint8_t *qtakes = nullptr;        // [nq] "the query's match blocks its slot" (nullptr: all do)
    int nq = 0;
    // the frame searched, its keypoint count, the slots that hold a point from the start (by keypoint index), the windows' stereo test
    FrameSrc *fs = nullptr;
    int n = 0;
    const uint8_t *occupied = nullptr;
    int has_uright = 0;
    // the rule.  mode 0: projection family / BoW lists; mode 1: SearchForInitialization (no accept_mode, no takes, no match_kp)
    int mode = 0, th = 0;
    float nnratio = 0.f;
    int accept_mode = ACCEPT_BEST, check = 0;       // check: the rotation-consistency check
    // the results: match_kp [n], match_q [nq], the count
    int32_t *match_kp = nullptr, *match_q = nullptr;
    int *nmatches = nullptr;
    WinQuery *queries_out = nullptr;
    SearchChain *chain = nullptr;           // work appended behind the resolver, in front of the wait (mode 0 on a prefix, one segment)
    bool sequential = false;                // start on the sequential resolver (a search whose fixed point is known not to settle)
    int *waits = nullptr;                   // optional: counts the call's host waits
    bool windows() const { return queries || prefix; }
};

// What the retry loop carries from attempt to attempt.
struct SeqPlan {
    bool exact = false;         // window lists by count, scan, fill (a strided attempt overflowed)
    bool sized = false;         // ... whose total has been read once
    bool sequential = false;    // k_resolve + k_rotation instead of the parallel fixed point
    size_t ent_need = 0;        // candidate entries
    int win_stride = 0, init_c = 0, gen = 0;
    int waits = 0;              // host waits of the call so far (orbm_debug_last_search_waits)
    size_t lds = 0;             // k_resolve's state
    bool fused_upload = false;  // the prefix kernel uploads the staged block
    const int *lbeg = nullptr, *lend = nullptr;     // every query's list bounds in w.ent, as the list kernels leave them
};

// Workspace offsets of one attempt: the staged inputs (same offsets in the pinned and the device arena: ONE upload), the prefix's
// inputs (read where they are staged), device-only arrays, then the result block [o_res, ...): the search's results, the chain's.
struct SeqLayout {
    size_t o_qh, o_a, o_qang, o_tk, o_occ, o_off, o_cbeg, o_cand, o_seg, o_ovf, staged;
    size_t o_q, o_top, o_cnt, o_acc, o_lend, o_state;
    size_t o_res, o_mq, o_mk, o_nm, search_res_bytes;
    size_t tq_bytes, tp_bytes;      // optional outputs that are not part of the result block travel through the tail of the pinned arena
    char *tq_pin, *tp_pin;
    template <typename T> T *res(const Workspace &w, size_t o) const { return reinterpret_cast<T *>(w.pin + (o - o_res)); }   // a result, host side
};

int seq_check(const SeqSearch &r)
{
    if (r.fs->ns() > SEQ_MAXN || r.nq > 65536) ORBX_FAIL(ORBX_ERR_CAPACITY, "frame too large for the sequential resolver");
    if (r.mode != 0 && r.lists.seg) ORBX_FAIL(ORBX_ERR_ARG, "SearchForInitialization does not resolve in segments");
    if (r.chain && (r.mode != 0 || r.lists.seg || !r.prefix)) ORBX_FAIL(ORBX_ERR_ARG, "a chain follows a whole-function projection search only");
    return ORBX_OK;
}

int seq_layout(const SeqSearch &r, Workspace &w, const SeqPlan &p, SeqLayout &L)
{
    const int nq = r.nq, ns = r.fs->ns(), n = r.n;
    w.used = 0;
    L.o_qh = w.carve(r.queries ? sizeof(WinQuery) * nq : 1);
    L.o_a = w.carve(r.q.frame ? sizeof(int) * (size_t)nq : (size_t)32 * nq);
    r.fs->carve(w);
    L.o_qang = w.carve(sizeof(float) * nq); L.o_tk = w.carve(nq); L.o_occ = w.carve(r.occupied && ns ? (size_t)ns : 1);
    L.o_off = w.carve(sizeof(int) * (nq + 1));
    L.o_cbeg = w.carve(sizeof(int) * (size_t)nq); L.o_cand = w.carve(sizeof(int) * (size_t)(r.lists.n ? r.lists.n : 1));
    L.o_seg = w.carve(sizeof(int) * (size_t)(r.lists.nseg + 1));
    L.o_ovf = w.carve(sizeof(int));                 // "a list outgrew its region": staged as 0, raised by k_win_wave<2>
    if (r.chain) r.chain->carve_inputs(w);
    L.staged = w.used;
    if (r.prefix) r.prefix->carve(w);              // read by the prefix kernel where they are staged: not part of the upload
    const size_t pin_in = w.used;
    if (r.prefix) r.prefix->carve_scratch(w);
    const size_t o_qd = w.carve(r.queries ? 1 : sizeof(WinQuery) * nq);
    L.o_q = r.queries ? L.o_qh : o_qd;
    L.o_top = w.carve(sizeof(unsigned) * TOPK * (size_t)nq); L.o_cnt = w.carve(sizeof(int) * nq); L.o_acc = w.carve(sizeof(int) * nq);
    L.o_lend = w.carve(sizeof(int) * nq);
    L.o_state = w.carve(sizeof(int) * (size_t)std::max(std::max(ns, nq), 1));
    L.o_res = w.used;
    L.o_mq = w.carve(sizeof(int) * nq); L.o_mk = w.carve(sizeof(int) * (size_t)(n ? n : 1)); L.o_nm = w.carve(4 * sizeof(int));
    L.search_res_bytes = w.used - L.o_res;
    if (r.chain) r.chain->carve_results(w);
    const size_t total_bytes = w.used, res_bytes = total_bytes - L.o_res;
    L.tq_bytes = r.queries_out ? (sizeof(WinQuery) * nq + 255) & ~(size_t)255 : 0;
    L.tp_bytes = r.prefix && r.prefix->frustum && r.prefix->proj_host ? (sizeof(orbm_projected_point) * (size_t)nq + 255) & ~(size_t)255 : 0;
    if (w.reserve(total_bytes, std::max(pin_in, res_bytes) + L.tq_bytes + L.tp_bytes)) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    L.tq_pin = w.pin + w.pin_cap - L.tq_bytes; L.tp_pin = L.tq_pin - L.tp_bytes;
    if (w.reserve_entries(p.ent_need)) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    return ORBX_OK;
}

// The inputs into the pinned arena, their upload (one copy, or left to the prefix kernel's launch), the presets, the prefix
// kernel and the copies of its optional outputs.
int seq_stage(const SeqSearch &r, Workspace &w, const SeqLayout &L, SeqPlan &p)
{
    const int nq = r.nq, ns = r.fs->ns();
    hipStream_t st = w.st;
    if (r.queries) memcpy(w.h<char>(L.o_qh), r.queries, sizeof(WinQuery) * nq);
    if (r.q.frame) memcpy(w.h<char>(L.o_a), r.q.pos, sizeof(int) * (size_t)nq);
    else memcpy(w.h<char>(L.o_a), r.q.desc, (size_t)32 * nq);
    r.fs->fill(w);
    if (!r.q.frame) {   // (from a resident frame: k_list_fill sets the angles down)
        if (r.q.angle) memcpy(w.h<char>(L.o_qang), r.q.angle, sizeof(float) * nq); else memset(w.h<char>(L.o_qang), 0, sizeof(float) * nq);
    }
    if (r.qtakes) memcpy(w.h<char>(L.o_tk), r.qtakes, nq); else memset(w.h<char>(L.o_tk), 1, nq);
    if (r.occupied && ns) r.fs->fill_occ(w.h<uint8_t>(L.o_occ), r.occupied);
    if (r.lists.off) {
        memcpy(w.h<char>(L.o_off), r.lists.off, sizeof(int) * (nq + 1));
        memcpy(w.h<char>(L.o_cbeg), r.lists.beg, sizeof(int) * (size_t)nq);
        if (r.lists.n) memcpy(w.h<char>(L.o_cand), r.lists.idx, sizeof(int) * r.lists.n);
    }
    if (r.lists.seg) memcpy(w.h<char>(L.o_seg), r.lists.seg, sizeof(int) * (size_t)(r.lists.nseg + 1));
    *w.h<int>(L.o_ovf) = 0;
    if (r.prefix) r.prefix->fill(w);
    if (r.chain) { r.chain->fill_inputs(w); r.chain->launched = false; }
    p.fused_upload = r.prefix && orbx::stage_ok(w.dev, w.pin, L.staged);
    if (!p.fused_upload) ORBX_HIP(orbx::stage_in(w.dev, w.pin, L.staged, st));
    // ONE fill for everything that needs a preset (a launch each was 3-4 us of a 0.1-ms call): match_kp = -1 (slot untouched);
    // segments write back touched slots of the state only, so it is preset to -1 as well (the span in between, match_q, is
    // rewritten in full anyway); and the two counters START AT -1: the match count is overwritten (one workgroup) or added
    // to (segments: the host adds the 1 back).  k_resolve_par writes every slot and its count itself.  The two flags are this
    // call's generation number when raised, and neither relies on what the arena held: "the fixed point was reached" is written
    // either way (0 or the generation) by the resolver, and "a list outgrew its region", which k_win_wave<2> writes only when a
    // list overflows, lies in the staged block (o_ovf), where the call's one upload sets it to 0 -- a word left by an earlier call
    // may equal this generation, so a flag that is only ever raised must not start from stale memory
    p.gen = (int)w.begin_generation();
    if (p.sequential) {
        const size_t f0 = r.lists.seg ? L.o_state : L.o_mk;
        ORBX_HIP(hipMemsetAsync(w.d<char>(f0), 0xff, L.o_nm + sizeof(int) - f0, st));
    }
    WinQuery *dq = w.d<WinQuery>(L.o_q);
    if (r.prefix) r.prefix->launch(w, dq, st, p.fused_upload ? stage_job(w.dev, w.pin, L.staged) : StageJob{nullptr, nullptr, 0, 0});
    if (L.tq_bytes) ORBX_HIP(hipMemcpyAsync(L.tq_pin, dq, sizeof(WinQuery) * nq, hipMemcpyDeviceToHost, st));
    if (L.tp_bytes) ORBX_HIP(hipMemcpyAsync(L.tp_pin, w.d<char>(r.prefix->o_proj), sizeof(orbm_projected_point) * (size_t)nq, hipMemcpyDeviceToHost, st));
    return ORBX_OK;
}

// Every query's candidate list with its distances and its short list: explicit lists, or window lists.  Window lists: their
// lengths are known only on the device.  First attempt: every query fills its own region of win_stride entries in one pass (no
// count, no scan, no host wait); if a list does not fit, the overflow flag comes back with the results and the call is repeated
// on the exact path (count, scan, fill), whose total is needed to size the buffer: the one extra host wait of that (rare) path.
int seq_lists(const SeqSearch &r, Workspace &w, const SeqLayout &L, SeqPlan &p)
{
    const int nq = r.nq;
    hipStream_t st = w.st;
    const FrameView fv = r.fs->view(w);
    const WinQuery *dq = w.d<WinQuery>(L.o_q);
    const uint4 *da = w.d<uint4>(L.o_a);
    const uint8_t *docc = r.occupied ? w.d<uint8_t>(L.o_occ) : nullptr;
    int *doff = w.d<int>(L.o_off), *dnm = w.d<int>(L.o_nm);
    unsigned *dtop = w.d<unsigned>(L.o_top);
    const int init_dist = r.mode == 0 ? 256 : INT_MAX;
    const dim3 g((nq + MT / 64 - 1) / (MT / 64)); // one wave per query
    p.lbeg = doff; p.lend = doff + 1;             // CSR lists; the strided path has its own bounds
    if (!r.windows()) {
        const orbm_frame *qf = r.q.frame;
        hipLaunchKernelGGL(k_list_fill, g, dim3(MT), 0, st, qf ? (const uint4 *)qf->desc : da, nq, fv.desc, (const int *)doff,
                           (const int *)w.d<int>(L.o_cbeg), (const int *)w.d<int>(L.o_cand), w.ent, dtop,
                           qf ? (const int *)w.d<int>(L.o_a) : (const int *)nullptr, qf ? (const float *)qf->angle : (const float *)nullptr,
                           w.d<float>(L.o_qang));
    } else if (!p.exact) {
        p.lbeg = w.d<int>(L.o_cnt); p.lend = w.d<int>(L.o_lend);
        hipLaunchKernelGGL(k_win_wave<2>, g, dim3(MT), 0, st, dq, da, nq, fv.kp, fv.desc, fv.cell_off, docc, fv.gp, r.has_uright,
                           init_dist, (int *)nullptr, (const int *)nullptr, w.ent, p.win_stride, w.d<int>(L.o_cnt), w.d<int>(L.o_lend), w.d<int>(L.o_ovf), dtop, p.gen);
    } else {
        hipLaunchKernelGGL(k_win_wave<0>, g, dim3(MT), 0, st, dq, da, nq, fv.kp, fv.desc, fv.cell_off, docc, fv.gp, r.has_uright,
                           init_dist, w.d<int>(L.o_cnt), (const int *)nullptr, (unsigned *)nullptr, 0, (int *)nullptr, (int *)nullptr,
                           (int *)nullptr, (unsigned *)nullptr, p.gen);
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(MT), 0, st, (const int *)w.d<int>(L.o_cnt), nq, doff, dnm + 1);
        if (!p.sized) {
            p.sized = true;
            int total = 0;
            ORBX_HIP(hipMemcpyAsync(&total, dnm + 1, sizeof(int), hipMemcpyDeviceToHost, st));
            ORBX_HIP(hipStreamSynchronize(st));
            if (r.chain) r.chain->waits++;
            ++p.waits;
            p.ent_need = (size_t)total;
            if (w.reserve_entries(p.ent_need)) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
        }
        hipLaunchKernelGGL(k_win_wave<1>, g, dim3(MT), 0, st, dq, da, nq, fv.kp, fv.desc, fv.cell_off, docc, fv.gp, r.has_uright,
                           init_dist, (int *)nullptr, (const int *)doff, w.ent, 0, (int *)nullptr, (int *)nullptr, (int *)nullptr, dtop, p.gen);
    }
    return ORBX_OK;
}

// The resolver.  The projection family and the BoW lists (mode 0) resolve as a parallel fixed point with the rotation check
// fused (k_resolve_par), SearchForInitialization (mode 1) likewise (k_resolve_init_par: its per-slot acceptor lists take
// init_c + 3 ints of LDS per keypoint); these write the result block in pinned memory themselves.  p.sequential: the one-wave
// sequential resolver and k_rotation, then the copy of the result block.  (The BoW searches' segments -- one per vocabulary
// node -- only matter to the sequential resolver: the fixed point needs no partition, queries of different nodes never meet.)
int seq_resolve(const SeqSearch &r, Workspace &w, const SeqLayout &L, const SeqPlan &p)
{
    const int nq = r.nq, ns = r.fs->ns();
    hipStream_t st = w.st;
    const FrameView fv = r.fs->view(w);
    const unsigned *dent = w.ent, *dtop = w.d<unsigned>(L.o_top);
    const float *dqang = w.d<float>(L.o_qang);
    const uint8_t *dtk = w.d<uint8_t>(L.o_tk);
    int *dnm = w.d<int>(L.o_nm);
    const int *dovf = r.windows() && !p.exact ? w.d<int>(L.o_ovf) : nullptr;    // only the strided window lists can overflow
    if (!p.sequential && r.mode == 1) {
        hipLaunchKernelGGL(k_resolve_init_par, dim3(1), dim3(RES_T), sizeof(int) * (size_t)(p.init_c + 3) * ns, st, dent, dtop, p.lbeg, p.lend,
                           nq, ns, p.init_c, r.th, r.nnratio, dqang, fv.angle, fv.perm, r.check, w.d<unsigned>(L.o_acc), dovf, p.gen,
                           L.res<int>(w, L.o_mq), L.res<int>(w, L.o_nm));
    } else if (!p.sequential) {
        hipLaunchKernelGGL(k_resolve_par, dim3(1), dim3(RES_T), sizeof(int) * 4 * (size_t)ns, st, dent, dtop, p.lbeg, p.lend, nq, ns, dtk, r.th,
                           r.nnratio, r.accept_mode, dqang, fv.angle, fv.perm, r.check, w.d<int>(L.o_mq), w.d<int>(L.o_mk), r.n, dovf,
                           p.gen, L.res<int>(w, L.o_mq), L.res<int>(w, L.o_mk), L.res<int>(w, L.o_nm), dnm);
    } else {
        const int *dseg = r.lists.seg ? w.d<int>(L.o_seg) : nullptr;
        const dim3 gr(r.lists.seg ? r.lists.nseg : 1);
        int *dacc = w.d<int>(L.o_acc), *dstate = w.d<int>(L.o_state);
        if (r.mode == 0) {
            hipLaunchKernelGGL(k_resolve<0>, gr, dim3(64), p.lds, st, dent, dtop, p.lbeg, p.lend, nq, ns, dtk, r.th, r.nnratio, r.accept_mode,
                               dacc, dstate, dnm, dseg);
            hipLaunchKernelGGL(k_rotation<0>, dim3(1), dim3(MT), 0, st, (const int *)dacc, (const int *)dstate, nq, ns, dqang, fv.angle,
                               fv.perm, r.check, w.d<int>(L.o_mq), w.d<int>(L.o_mk), dnm, dovf);
        } else {
            hipLaunchKernelGGL(k_resolve<1>, gr, dim3(64), p.lds, st, dent, dtop, p.lbeg, p.lend, nq, ns, dtk, r.th, r.nnratio, 0,
                               dacc, dstate, dnm, dseg);
            hipLaunchKernelGGL(k_rotation<1>, dim3(1), dim3(MT), 0, st, (const int *)dacc, (const int *)dstate, nq, ns, dqang, fv.angle,
                               fv.perm, r.check, w.d<int>(L.o_mq), w.d<int>(L.o_mk), dnm, dovf);
        }
    }
    ORBX_HIP(hipGetLastError());
    if (p.sequential) ORBX_HIP(orbx::stage_out(w.pin, w.dev + L.o_res, L.search_res_bytes, st));
    return ORBX_OK;
}

// The results of the attempt that stands, from the pinned arena to the caller's arrays (searched = false: the prefix's only).
void seq_collect(const SeqSearch &r, const Workspace &w, const SeqLayout &L, const SeqPlan &p, bool searched)
{
    const int nq = r.nq;
    if (searched) {
        memcpy(r.match_q, L.res<char>(w, L.o_mq), sizeof(int) * nq);
        if (r.mode == 0 && r.n) memcpy(r.match_kp, L.res<char>(w, L.o_mk), sizeof(int) * r.n);
        memcpy(r.nmatches, L.res<char>(w, L.o_nm), sizeof(int));
        if (r.lists.seg && p.sequential) *r.nmatches += 1;   // the segments added their counts to the preset -1
    }
    if (L.tq_bytes) memcpy(r.queries_out, L.tq_pin, sizeof(WinQuery) * nq);
    if (L.tp_bytes) memcpy(r.prefix->proj_host, L.tp_pin, sizeof(orbm_projected_point) * (size_t)nq);
}

// The LDS limits of the five resolvers (the largest request each can make; the fixed-point kernels also have static LDS), raised
// once per process whichever thread calls first.  A failure stays and fails every call.
int resolver_lds_limits()
{
    static const hipError_t err = [] {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (!e) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (!e) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_par), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (!e) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_init_par), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (!e) e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_par_pairs), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        return e;
    }();
    ORBX_HIP(err);
    return ORBX_OK;
}

// Inputs are staged in the workspace's pinned arena and uploaded with one copy; results come back in one block.  Everything
// runs on the workspace's stream, and the host waits ONCE, at the end of an attempt.  An attempt is repeated when its flags,
// which come back with the results, say so: a window list outgrew its region (strided -> exact lists), or the fixed point did
// not settle (parallel -> sequential resolver: the result never depends on how the dependency chains fall).
int run_sequential(const SeqSearch &r)
{
    if (const int rc = seq_check(r)) return rc;
    const int ns = r.fs->ns(), nq = r.nq;
    for (int j = 0; j < r.n && r.mode == 0; ++j) r.match_kp[j] = -1;
    for (int i = 0; i < nq; ++i) r.match_q[i] = -1;
    *r.nmatches = 0;
    if (r.queries_out) for (int i = 0; i < nq; ++i) r.queries_out[i] = {0.f, 0.f, -1.f, 0.f, 0, -1};
    if (nq == 0 || (ns == 0 && !r.queries_out && !(r.prefix && r.prefix->proj_host))) return ORBX_OK;
    SeqPlan p;
    p.lds = sizeof(int) * (3 * (size_t)ns + (r.mode == 1 ? nq : 0)) + 16;
    if (p.lds > 160 * 1024) ORBX_FAIL(ORBX_ERR_CAPACITY, "resolver state exceeds LDS");
    // (SearchForInitialization's windows are 200 px wide: a few hundred candidates each, where the projection searches see tens)
    p.win_stride = r.mode == 1 ? 1024 : 256;
    p.ent_need = r.lists.off ? (size_t)r.lists.off[nq] : (size_t)nq * p.win_stride;
    p.init_c = ns ? std::min(7, (144 * 1024 / 4) / ns - 3) : 7;
    p.sequential = r.sequential || g_force_sequential.load(std::memory_order_relaxed) != 0 || (r.mode == 1 && p.init_c < 2);

    WorkspaceLease lease;
    Workspace &w = *lease.w;
    if (const int rc = resolver_lds_limits()) return rc;
    for (int attempt = 0; attempt < 4; ++attempt) {
        SeqLayout L;
        if (const int rc = seq_layout(r, w, p, L)) return rc;
        if (const int rc = seq_stage(r, w, L, p)) return rc;
        if (ns) {
            if (const int rc = seq_lists(r, w, L, p)) return rc;
            if (const int rc = seq_resolve(r, w, L, p)) return rc;
        }               // (else nothing to search: the prefix's outputs are the whole result)
        const SearchChain::Ctx cx = {&w, w.st, w.d<int>(L.o_mk), w.d<int>(L.o_nm), w.d<int>(L.o_ovf), w.d<uint8_t>(L.o_tk), r.n, nq, p.gen, r.windows() && !p.exact,
                                     !p.sequential, L.o_res};
        if (r.chain && ns) {    // its kernel reads the flags the host reads below, and leaves if this attempt does not stand
            if (const int rc = r.chain->launch(cx)) return rc;
            r.chain->launched = true;
        }
        ORBX_HIP(hipStreamSynchronize(w.st));
        if (r.chain) r.chain->waits++;
        if (r.waits) ++*r.waits;
        g_last_search_waits.store(++p.waits, std::memory_order_relaxed);
        if (ns) {
            if (r.windows() && !p.exact && *L.res<int>(w, L.o_nm + sizeof(int)) == p.gen) { p.exact = true; continue; }
            if (!p.sequential) {
                const int conv = *L.res<int>(w, L.o_nm + 2 * sizeof(int));
                g_last_iterations.store(conv == p.gen ? *L.res<int>(w, L.o_nm + 3 * sizeof(int)) : -1, std::memory_order_relaxed);
                if (conv != p.gen) { p.sequential = true; continue; }
            }
        }
        seq_collect(r, w, L, p, ns != 0);
        if (r.chain && ns) r.chain->collect(cx);
        break;
    }
    return ORBX_OK;
}

// orbm_search_projection on a frame from either source: the caller's windows, the loop of SearchByProjection (:69-130)
int search_projection_core(FrameSrc &fs, int n, int has_uright, const orbm_window_query *queries, const uint8_t *qdesc, const float *qangle,
                           const uint8_t *qtakes, int nq, const uint8_t *occupied, int th_accept, float nnratio, int ratio_same_level,
                           int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches)
{
    SeqSearch r;
    r.queries = reinterpret_cast<const WinQuery *>(queries); r.q.desc = qdesc; r.q.angle = qangle; r.qtakes = qtakes; r.nq = nq;
    r.fs = &fs; r.n = n; r.occupied = occupied; r.has_uright = has_uright;
    r.th = th_accept; r.nnratio = nnratio; r.accept_mode = ratio_same_level ? ACCEPT_RATIO_SAME_LEVEL : ACCEPT_BEST; r.check = check_orientation;
    r.match_kp = match_kp; r.match_q = match_q; r.nmatches = nmatches;
    return run_sequential(r);
}

int search_init_core(FrameSrc &fs, int n2, const orbx_keypoint *kps2, const orbx_keypoint *kps1, const uint8_t *desc1, int n1, float *prev_matched, int window_size,
                     float nnratio, int check_orientation, int32_t *matches12, int *nmatches)
{
    // queries: level-0 keypoints of F1 around their previous match (:619-626); others get an empty window
    std::vector<WinQuery> q(n1 ? n1 : 1);
    std::vector<float> ang(n1 ? n1 : 1);
    for (int i = 0; i < n1; ++i) {
        const bool use = !(kps1[i].octave > 0);
        q[i] = {prev_matched[2 * i], prev_matched[2 * i + 1], use ? (float)window_size : -1.0f, 0.f, kps1[i].octave, kps1[i].octave};
        ang[i] = kps1[i].angle;
    }
    SeqSearch r;
    r.queries = q.data(); r.q.desc = desc1; r.q.angle = ang.data(); r.nq = n1;
    r.fs = &fs; r.n = n2;
    r.mode = 1; r.th = 45 /* TH_LOW, :38 */; r.nnratio = nnratio; r.check = check_orientation;
    r.match_q = matches12; r.nmatches = nmatches;
    const int rc = run_sequential(r);
    for (int i = 0; i < n1 && rc == ORBX_OK; ++i) // :715-718
        if (matches12[i] >= 0) { prev_matched[2 * i] = kps2[matches12[i]].x; prev_matched[2 * i + 1] = kps2[matches12[i]].y; }
    return rc;
}

} // namespace

extern "C" {

int orbm_debug_force_sequential_resolver(int on)
{
    return g_force_sequential.exchange(on ? 1 : 0, std::memory_order_relaxed);
}

int orbm_debug_last_resolver_iterations(void) { return g_last_iterations.load(std::memory_order_relaxed); }
int orbm_debug_last_search_waits(void) { return g_last_search_waits.load(std::memory_order_relaxed); }

int orbm_project_points(int mode, const float *mp_pos, const float *mp_normal, const float *mp_min_distance,
                        const float *mp_max_distance, int m, const float *Rcw, const float *tcw, const float *Ow,
                        const orbm_camera *cam, float mbf, float viewing_cos_limit, float log_scale_factor,
                        const float *scale_factors, int nlevels, float th, orbm_projected_point *out, orbm_window_query *queries)
{
    if (mode < 0 || mode > 2 || m < 0 || nlevels < 1 || nlevels > 64 || !cam || !Rcw || !tcw || !Ow || !scale_factors || !out ||
        (m && (!mp_pos || !mp_normal || !mp_min_distance || !mp_max_distance)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    if (m == 0) return ORBX_OK;
    StagedCall sc;
    const size_t o_pos = sc.in(mp_pos, sizeof(float) * 3 * m), o_nrm = sc.in(mp_normal, sizeof(float) * 3 * m),
                 o_min = sc.in(mp_min_distance, sizeof(float) * m), o_max = sc.in(mp_max_distance, sizeof(float) * m),
                 o_sc = sc.in(scale_factors, sizeof(float) * nlevels);
    const size_t o_out = sc.out(sizeof(orbm_projected_point) * (size_t)m), o_q = sc.out(sizeof(WinQuery) * (size_t)m);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    ProjectCam pc;
    pc.fx = cam->fx; pc.fy = cam->fy; pc.cx = cam->cx; pc.cy = cam->cy;
    // Frame::isInFrustum compares with the grid bounds mnMinX..mnMaxY (static floats), KeyFrame::IsInImage likewise
    pc.min_x = cam->grid_min_x; pc.max_x = cam->grid_max_x; pc.min_y = cam->grid_min_y; pc.max_y = cam->grid_max_y;
    pc.mbf = mbf; pc.cos_limit = viewing_cos_limit; pc.log_scale = log_scale_factor; pc.th = th;
    for (int i = 0; i < 9; ++i) pc.R[i] = Rcw[i];
    for (int i = 0; i < 3; ++i) { pc.t[i] = tcw[i]; pc.Ow[i] = Ow[i]; }
    pc.nlevels = nlevels; pc.mode = mode;
    hipLaunchKernelGGL(k_project_points, dim3((m + MT - 1) / MT), dim3(MT), 0, sc.stream(), (const uint8_t *)nullptr, sc.d<const float>(o_pos),
                       sc.d<const float>(o_nrm), sc.d<const float>(o_min), sc.d<const float>(o_max), m, pc, sc.d<const float>(o_sc),
                       sc.d<orbm_projected_point>(o_out), sc.d<WinQuery>(o_q), StageJob{nullptr, nullptr, 0, 0});
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    memcpy(out, sc.r<orbm_projected_point>(o_out), sizeof(orbm_projected_point) * (size_t)m);
    if (queries) memcpy(queries, sc.r<WinQuery>(o_q), sizeof(WinQuery) * (size_t)m);
    return ORBX_OK;
}

int orbm_search_projection(const orbm_window_query *queries, const uint8_t *qdesc, const float *qangle, const uint8_t *qtakes,
                           int nq, const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *occupied,
                           const float *uright, float min_x, float min_y, float max_x, float max_y, int th_accept, float nnratio,
                           int ratio_same_level, int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches)
{
    if (nq < 0 || n < 0 || n > 65535 || (nq && (!queries || !qdesc || !match_q)) || (n && (!kps || !desc || !match_kp)) || !nmatches ||
        (check_orientation && nq && !qangle) || !(max_x > min_x) || !(max_y > min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(kps, n)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    SortedFrame sf;
    sort_frame(kps, desc, n, nullptr, uright, min_x, min_y, max_x, max_y, sf);
    FrameSrc fs(sf);
    return search_projection_core(fs, n, uright ? 1 : 0, queries, qdesc, qangle, qtakes, nq, occupied, th_accept, nnratio, ratio_same_level,
                                  check_orientation, match_kp, match_q, nmatches);
}

int orbm_frame_search_projection(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, const float *qangle,
                                 const uint8_t *qtakes, int nq, const uint8_t *occupied, int th_accept, float nnratio, int ratio_same_level,
                                 int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches)
{
    if (!frame || nq < 0 || (nq && (!queries || !qdesc || !match_q)) || (frame->n && !match_kp) || !nmatches || (check_orientation && nq && !qangle))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(frame)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    FrameSrc fs(frame);
    return search_projection_core(fs, frame->n, frame->has_uright, queries, qdesc, qangle, qtakes, nq, occupied, th_accept, nnratio,
                                  ratio_same_level, check_orientation, match_kp, match_q, nmatches);
}

int orbm_search_for_initialization(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbx_keypoint *kps2,
                                   const uint8_t *desc2, int n2, float *prev_matched, float min_x, float min_y, float max_x,
                                   float max_y, int window_size, float nnratio, int check_orientation, int32_t *matches12,
                                   int *nmatches)
{
    if (n1 < 0 || n2 < 0 || n2 > 65535 || (n1 && (!kps1 || !desc1 || !prev_matched || !matches12)) || (n2 && (!kps2 || !desc2)) ||
        !nmatches || !(max_x > min_x) || !(max_y > min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(kps2, n2)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    SortedFrame sf;
    sort_frame(kps2, desc2, n2, nullptr, nullptr, min_x, min_y, max_x, max_y, sf);
    FrameSrc fs(sf);
    return search_init_core(fs, n2, kps2, kps1, desc1, n1, prev_matched, window_size, nnratio, check_orientation, matches12, nmatches);
}

int orbm_frame_search_for_initialization(const orbm_frame *frame2, const orbx_keypoint *kps2, const orbx_keypoint *kps1, const uint8_t *desc1,
                                         int n1, float *prev_matched, int window_size, float nnratio, int check_orientation,
                                         int32_t *matches12, int *nmatches)
{
    if (!frame2 || n1 < 0 || (frame2->n && !kps2) || (n1 && (!kps1 || !desc1 || !prev_matched || !matches12)) || !nmatches)
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(frame2)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    FrameSrc fs(frame2);
    return search_init_core(fs, frame2->n, kps2, kps1, desc1, n1, prev_matched, window_size, nnratio, check_orientation, matches12, nmatches);
}

} // extern "C"

namespace {

// The co-iteration of the two FeatureVectors (ORBmatcher.cc:384-456 / :745-828: equal keys: visit; else lower_bound on the other
// map) as lists: every valid feature of a common node is a query whose candidates are that node's valid members in the other set, one
// copy per node.  inv2: candidate numbers are positions in a resident frame instead of feature indices.
struct BowLists {
    std::vector<int32_t> qidx, cand_off, cand_beg, cand, seg;
    bool disjoint = true;   // a feature sits in one node of a FeatureVector; arrays that break this resolve as one segment
    SeqSearch::Lists lists() const
    {
        SeqSearch::Lists l;
        l.off = cand_off.data(); l.beg = cand_beg.data(); l.idx = cand.data(); l.n = (int)cand.size();
        if (disjoint) { l.seg = seg.data(); l.nseg = (int)seg.size() - 1; }
        return l;
    }
};
void bow_lists(const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1, const uint8_t *valid1, const int32_t *nodes2,
               const int32_t *off2, const int32_t *items2, int nn2, const uint8_t *valid2, int n2, const int *inv2, BowLists &L)
{
    const size_t m1 = nn1 ? (size_t)off1[nn1] : 0, m2 = nn2 ? (size_t)off2[nn2] : 0;
    L.qidx.reserve(m1); L.cand_beg.reserve(m1); L.cand_off.reserve(m1 + 1); L.cand.reserve(m2); L.seg.reserve((size_t)std::min(nn1, nn2) + 1);
    L.cand_off.assign(1, 0); L.seg.assign(1, 0);
    std::vector<uint8_t> seen(n2 ? n2 : 1, 0);
    for_each_common_node(nodes1, nn1, nodes2, nn2, [&](int a, int b) {
        const size_t c0 = L.cand.size();
        for (int k = off2[b]; k < off2[b + 1]; ++k) { L.disjoint = L.disjoint && !seen[items2[k]]; seen[items2[k]] = 1; }
        for (int k = off2[b]; k < off2[b + 1]; ++k)
            if (!valid2 || valid2[items2[k]]) L.cand.push_back(inv2 ? inv2[items2[k]] : items2[k]);
        const int32_t len = (int32_t)(L.cand.size() - c0);
        bool any = false;
        for (int k = off1[a]; k < off1[a + 1]; ++k) { // every query of the node: the same members, one copy
            if (!valid1[items1[k]]) continue;
            any = true;
            L.qidx.push_back(items1[k]);
            L.cand_beg.push_back((int32_t)c0);
            L.cand_off.push_back(L.cand_off.back() + len);
        }
        if (!any) L.cand.resize(c0);
        else L.seg.push_back((int32_t)L.qidx.size());   // one segment per node
    });
}

// The arguments of one BoW search over two resident frames, as orbm_frame_search_by_bow and every pair of
// orbm_frame_search_by_bow_pairs are checked.
int bow_frames_check(const orbm_frame *frame1, const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1, const uint8_t *valid1,
                     const orbm_frame *frame2, const int32_t *nodes2, const int32_t *off2, const int32_t *items2, int nn2, const int32_t *match12)
{
    if (!frame1 || !frame2 || nn1 < 0 || nn2 < 0 || (frame1->n && (!match12 || !valid1)) || (nn1 && (!nodes1 || !off1 || !items1)) ||
        (nn2 && (!nodes2 || !off2 || !items2)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bow_check_items(off1, items1, nn1, frame1->n) || bow_check_items(off2, items2, nn2, frame2->n)) ORBX_FAIL(ORBX_ERR_ARG, "feature index out of range");
    return ORBX_OK;
}

// The match rows from a search's results: every accepted query blocks its candidate, so slot mq[i] still names i unless rejected.
void bow_rows(const BowLists &L, const int32_t *mq, const int32_t *mk, int32_t *match12, int32_t *match21)
{
    for (size_t i = 0; i < L.qidx.size(); ++i)
        if (mq[i] >= 0 && mk[mq[i]] == (int32_t)i) { match12[L.qidx[i]] = mq[i]; if (match21) match21[mq[i]] = L.qidx[i]; }
}

// One search over two resident frames whose lists hold a query, by run_sequential (rows preset by the caller).
int bow_frames_run(const orbm_frame *frame1, const orbm_frame *frame2, const BowLists &L, int th, int strict_th, float nnratio,
                   int check_orientation, bool sequential, int32_t *match12, int32_t *match21, int *nmatches, int *waits = nullptr)
{
    const int nq = (int)L.qidx.size(), n2 = frame2->n;
    std::vector<int32_t> qsrc(nq), mk(n2), mq(nq);
    for (int i = 0; i < nq; ++i) qsrc[i] = frame1->inv_host[L.qidx[i]];
    FrameSrc fs(frame2, true);
    SeqSearch r;
    r.lists = L.lists(); r.q.frame = frame1; r.q.pos = qsrc.data(); r.nq = nq;
    r.fs = &fs; r.n = n2;
    r.th = strict_th ? th - 1 : th; r.nnratio = nnratio; r.accept_mode = ACCEPT_RATIO; r.check = check_orientation;
    r.match_kp = mk.data(); r.match_q = mq.data(); r.nmatches = nmatches; r.sequential = sequential; r.waits = waits;
    const int rc = run_sequential(r);
    if (rc != ORBX_OK) return rc;
    bow_rows(L, mq.data(), mk.data(), match12, match21);
    return ORBX_OK;
}

// ---- orbm_frame_search_by_bow_pairs: K searches, one lease, one staged upload, one launch per phase, one host wait.
// The workspace of the batch: every search that has a query ("active") gets its regions behind each other.
struct BowBatchSlot {
    int pair = 0;                       // index in the caller's array
    BowLists L;
    std::vector<int32_t> qsrc;
    size_t o_qmap = 0, o_off = 0, o_cbeg = 0, o_cand = 0;       // staged
    size_t o_top = 0, o_qang = 0, o_mq = 0, o_mk = 0, o_nm = 0; // device only
    size_t o_hq = 0, o_hk = 0, o_hnm = 0;                       // result block (pinned: offset - o_res)
    size_t ent0 = 0;
};

int bow_pairs_launch(const orbm_bow_pair *pairs, std::vector<BowBatchSlot> &act, int th, int strict_th, float nnratio, int check_orientation,
                     int32_t *nmatches, std::vector<int> &unsettled, int &iterations, int &waits)
{
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    if (const int rc = resolver_lds_limits()) return rc;
    w.used = 0;
    size_t nent = 0;
    int max_nq = 0, max_ns = 0;
    for (BowBatchSlot &s : act) {
        const size_t nq = s.L.qidx.size(), nc = s.L.cand.size();
        s.o_qmap = w.carve(sizeof(int) * nq); s.o_off = w.carve(sizeof(int) * (nq + 1)); s.o_cbeg = w.carve(sizeof(int) * nq);
        s.o_cand = w.carve(sizeof(int) * (nc ? nc : 1));
        s.ent0 = nent; nent += ((size_t)s.L.cand_off[nq] + 63) & ~(size_t)63;
        max_nq = std::max(max_nq, (int)nq); max_ns = std::max(max_ns, pairs[s.pair].frame2->n);
    }
    const size_t o_rec = w.carve(sizeof(BowPairDev) * act.size());
    const size_t staged = w.used;
    for (BowBatchSlot &s : act) {
        const size_t nq = s.L.qidx.size(), n2 = (size_t)pairs[s.pair].frame2->n;
        s.o_top = w.carve(sizeof(unsigned) * TOPK * nq); s.o_qang = w.carve(sizeof(float) * nq);
        s.o_mq = w.carve(sizeof(int) * nq); s.o_mk = w.carve(sizeof(int) * n2); s.o_nm = w.carve(4 * sizeof(int));
    }
    const size_t o_res = w.used;
    for (BowBatchSlot &s : act) {
        const size_t nq = s.L.qidx.size(), n2 = (size_t)pairs[s.pair].frame2->n;
        s.o_hq = w.carve(sizeof(int) * nq); s.o_hk = w.carve(sizeof(int) * n2); s.o_hnm = w.carve(4 * sizeof(int));
    }
    const size_t res_bytes = w.used - o_res;
    if (w.reserve(o_res + res_bytes, std::max(staged, res_bytes))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    if (w.reserve_entries(nent)) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    const int gen = (int)w.begin_generation();
    BowPairDev *rec = w.h<BowPairDev>(o_rec);
    for (size_t a = 0; a < act.size(); ++a) {
        const BowBatchSlot &s = act[a];
        const orbm_frame *f1 = pairs[s.pair].frame1, *f2 = pairs[s.pair].frame2;
        const size_t nq = s.L.qidx.size();
        memcpy(w.h<char>(s.o_qmap), s.qsrc.data(), sizeof(int) * nq);
        memcpy(w.h<char>(s.o_off), s.L.cand_off.data(), sizeof(int) * (nq + 1));
        memcpy(w.h<char>(s.o_cbeg), s.L.cand_beg.data(), sizeof(int) * nq);
        if (!s.L.cand.empty()) memcpy(w.h<char>(s.o_cand), s.L.cand.data(), sizeof(int) * s.L.cand.size());
        BowPairDev &d = rec[a];
        d.A = f1->desc; d.B = f2->desc; d.qang_src = f1->angle; d.kangle = f2->angle; d.perm = f2->perm;
        d.qmap = w.d<int>(s.o_qmap); d.off = w.d<int>(s.o_off); d.cbeg = w.d<int>(s.o_cbeg); d.cand = w.d<int>(s.o_cand);
        d.ent = w.ent + s.ent0; d.top = w.d<unsigned>(s.o_top); d.qang = w.d<float>(s.o_qang);
        d.match_q = w.d<int>(s.o_mq); d.match_kp = w.d<int>(s.o_mk); d.dev_nm = w.d<int>(s.o_nm);
        d.host_q = reinterpret_cast<int *>(w.pin + (s.o_hq - o_res)); d.host_kp = reinterpret_cast<int *>(w.pin + (s.o_hk - o_res));
        d.host_nm = reinterpret_cast<int *>(w.pin + (s.o_hnm - o_res));
        d.nq = (int)nq; d.ns = f2->n; d.n = f2->n; d.reserved = 0;
    }
    hipStream_t st = w.st;
    ORBX_HIP(orbx::stage_in(w.dev, w.pin, staged, st));
    const BowPairDev *drec = w.d<BowPairDev>(o_rec);
    hipLaunchKernelGGL(k_list_fill_pairs, dim3((max_nq + MT / 64 - 1) / (MT / 64), (unsigned)act.size()), dim3(MT), 0, st, drec);
    hipLaunchKernelGGL(k_resolve_par_pairs, dim3((unsigned)act.size()), dim3(RES_T), sizeof(int) * 4 * (size_t)max_ns, st, drec,
                       strict_th ? th - 1 : th, nnratio, check_orientation, gen);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipStreamSynchronize(st));
    ++waits;
    for (const BowBatchSlot &s : act) {
        const orbm_bow_pair &p = pairs[s.pair];
        const int *hq = reinterpret_cast<const int *>(w.pin + (s.o_hq - o_res)), *hk = reinterpret_cast<const int *>(w.pin + (s.o_hk - o_res)),
                  *hnm = reinterpret_cast<const int *>(w.pin + (s.o_hnm - o_res));
        if (hnm[2] != gen) { unsettled.push_back((int)(&s - act.data())); iterations = -1; continue; }
        if (iterations >= 0) iterations = std::max(iterations, hnm[3]);
        bow_rows(s.L, hq, hk, p.match12, p.match21);
        nmatches[s.pair] = hnm[0];
    }
    return ORBX_OK;
}

} // namespace

extern "C" {

int orbm_search_by_bow(const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1, const uint8_t *valid1,
                       const uint8_t *desc1, const float *angle1, int n1, const int32_t *nodes2, const int32_t *off2,
                       const int32_t *items2, int nn2, const uint8_t *valid2, const uint8_t *desc2, const float *angle2, int n2,
                       int th, int strict_th, float nnratio, int check_orientation, int32_t *match12, int32_t *match21,
                       int *nmatches)
{
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || (n1 && (!desc1 || !match12 || !valid1)) || (n2 && !desc2) ||
        (nn1 && (!nodes1 || !off1 || !items1)) || (nn2 && (!nodes2 || !off2 || !items2)) || !nmatches ||
        (check_orientation && n1 && n2 && (!angle1 || !angle2)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bow_check_items(off1, items1, nn1, n1) || bow_check_items(off2, items2, nn2, n2)) ORBX_FAIL(ORBX_ERR_ARG, "feature index out of range");
    ORBX_NEED_DEVICE();
    for (int i = 0; i < n1; ++i) match12[i] = -1;
    if (match21) for (int j = 0; j < n2; ++j) match21[j] = -1;
    *nmatches = 0;
    BowLists L;
    bow_lists(nodes1, off1, items1, nn1, valid1, nodes2, off2, items2, nn2, valid2, n2, nullptr, L);
    const int nq = (int)L.qidx.size();
    if (nq == 0 || n2 == 0) return ORBX_OK;
    SortedFrame sf; // the second set as it is: position = feature index
    sf.perm.resize(n2); sf.angle.resize(n2); sf.desc.assign(desc2, desc2 + (size_t)32 * n2);
    for (int j = 0; j < n2; ++j) { sf.perm[j] = j; sf.angle[j] = angle2 ? angle2[j] : 0.f; }
    std::vector<uint8_t> qd((size_t)32 * nq);
    std::vector<float> qa(nq);
    for (int i = 0; i < nq; ++i) { memcpy(&qd[32 * (size_t)i], desc1 + 32 * (size_t)L.qidx[i], 32); qa[i] = angle1 ? angle1[L.qidx[i]] : 0.f; }
    std::vector<int32_t> mk(n2), mq(nq);
    FrameSrc fs(sf);
    SeqSearch r;
    r.lists = L.lists(); r.q.desc = qd.data(); r.q.angle = qa.data(); r.nq = nq;
    r.fs = &fs; r.n = n2;
    r.th = strict_th ? th - 1 : th; r.nnratio = nnratio; r.accept_mode = ACCEPT_RATIO; r.check = check_orientation;   // bestDist1 < TH_LOW (:799) == bestDist1 <= TH_LOW - 1
    r.match_kp = mk.data(); r.match_q = mq.data(); r.nmatches = nmatches;
    const int rc = run_sequential(r);
    if (rc != ORBX_OK) return rc;
    for (int i = 0; i < nq; ++i) // every accepted query blocks its candidate, so slot mq[i] still names i unless rejected
        if (mq[i] >= 0 && mk[mq[i]] == i) { match12[L.qidx[i]] = mq[i]; if (match21) match21[mq[i]] = L.qidx[i]; }
    return ORBX_OK;
}

int orbm_frame_search_by_bow(const orbm_frame *frame1, const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1,
                             const uint8_t *valid1, const orbm_frame *frame2, const int32_t *nodes2, const int32_t *off2,
                             const int32_t *items2, int nn2, const uint8_t *valid2, int th, int strict_th, float nnratio,
                             int check_orientation, int32_t *match12, int32_t *match21, int *nmatches)
{
    if (!nmatches) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (const int rc = bow_frames_check(frame1, nodes1, off1, items1, nn1, valid1, frame2, nodes2, off2, items2, nn2, match12)) return rc;
    const int n1 = frame1->n, n2 = frame2->n;
    ORBX_NEED_DEVICE();
    for (int i = 0; i < n1; ++i) match12[i] = -1;
    if (match21) for (int j = 0; j < n2; ++j) match21[j] = -1;
    *nmatches = 0;
    BowLists L;
    bow_lists(nodes1, off1, items1, nn1, valid1, nodes2, off2, items2, nn2, valid2, n2, frame2->inv_host.data(), L);
    if (L.qidx.empty() || n2 == 0) return ORBX_OK;
    return bow_frames_run(frame1, frame2, L, th, strict_th, nnratio, check_orientation, false, match12, match21, nmatches);
}

int orbm_frame_search_by_bow_pairs(const orbm_bow_pair *pairs, int K, int th, int strict_th, float nnratio, int check_orientation,
                                   int32_t *nmatches)
{
    if (K < 0 || (K && (!pairs || !nmatches))) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (K > 64) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "at most 64 pairs per call");
    for (int k = 0; k < K; ++k) {
        const orbm_bow_pair &p = pairs[k];
        if (const int rc = bow_frames_check(p.frame1, p.nodes1, p.off1, p.items1, p.nn1, p.valid1, p.frame2, p.nodes2, p.off2, p.items2, p.nn2,
                                            p.match12))
            return rc;
        if (p.frame2->n > SEQ_MAXN) ORBX_FAIL(ORBX_ERR_CAPACITY, "frame too large for the resolver");
    }
    ORBX_NEED_DEVICE();
    g_last_bow_pairs_waits.store(0, std::memory_order_relaxed);
    std::vector<BowBatchSlot> act;
    act.reserve((size_t)K);
    for (int k = 0; k < K; ++k) {
        const orbm_bow_pair &p = pairs[k];
        const int n1 = p.frame1->n, n2 = p.frame2->n;
        for (int i = 0; i < n1; ++i) p.match12[i] = -1;
        if (p.match21) for (int j = 0; j < n2; ++j) p.match21[j] = -1;
        nmatches[k] = 0;
        act.emplace_back();
        BowBatchSlot &s = act.back();
        s.pair = k;
        bow_lists(p.nodes1, p.off1, p.items1, p.nn1, p.valid1, p.nodes2, p.off2, p.items2, p.nn2, p.valid2, n2, p.frame2->inv_host.data(), s.L);
        if (s.L.qidx.empty() || n2 == 0) { act.pop_back(); continue; }     // no query: the -1 rows stand, the pair takes no part in the launch
        s.qsrc.resize(s.L.qidx.size());
        for (size_t i = 0; i < s.qsrc.size(); ++i) s.qsrc[i] = p.frame1->inv_host[s.L.qidx[i]];
    }
    if (act.empty()) return ORBX_OK;
    int waits = 0;              // (counted here and published once: concurrent calls do not add to each other's count)
    std::vector<int> again;     // positions in act of the pairs that go through the single-pair path on the sequential resolver
    if (g_force_sequential.load(std::memory_order_relaxed) != 0) {
        for (size_t a = 0; a < act.size(); ++a) again.push_back((int)a);
    } else if (act.size() == 1) {   // a batch of one search IS the single call (its record costs the two kernels a dependent load each)
        const orbm_bow_pair &p = pairs[act[0].pair];
        const int rc = bow_frames_run(p.frame1, p.frame2, act[0].L, th, strict_th, nnratio, check_orientation, false, p.match12, p.match21,
                                      &nmatches[act[0].pair], &waits);
        g_last_bow_pairs_waits.store(waits, std::memory_order_relaxed);
        return rc;
    } else {
        int iterations = 0;
        if (const int rc = bow_pairs_launch(pairs, act, th, strict_th, nnratio, check_orientation, nmatches, again, iterations, waits)) return rc;
        g_last_iterations.store(iterations, std::memory_order_relaxed);
        g_last_bow_pairs_waits.store(waits, std::memory_order_relaxed);
    }
    for (const int a : again) {     // the other pairs' results stand; each of these costs one more wait
        const orbm_bow_pair &p = pairs[act[a].pair];
        if (const int rc = bow_frames_run(p.frame1, p.frame2, act[a].L, th, strict_th, nnratio, check_orientation, true, p.match12, p.match21,
                                          &nmatches[act[a].pair]))
            return rc;
        g_last_bow_pairs_waits.store(++waits, std::memory_order_relaxed);
    }
    return ORBX_OK;
}

int orbm_debug_last_bow_pairs_waits(void) { return g_last_bow_pairs_waits.load(std::memory_order_relaxed); }

// ------------------------------------------------------- the projection searches as whole functions, on resident frames

int orbm_search_by_projection_points(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *points,
                                     const uint8_t *occupied, float th, float viewing_cos_limit, int th_high, float nnratio, int32_t *match_kp,
                                     int32_t *match_q, int *nmatches, orbm_projected_point *projected_out, orbm_window_query *queries_out)
{
    return search_by_projection_points_chain(cur, view, Tcw, points, occupied, th, viewing_cos_limit, th_high, nnratio, match_kp, match_q,
                                             nmatches, projected_out, queries_out, nullptr);
}

} // extern "C"

int orbm_detail::search_by_projection_points_chain(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *points,
                                                   const uint8_t *occupied, float th, float viewing_cos_limit, int th_high, float nnratio,
                                                   int32_t *match_kp, int32_t *match_q, int *nmatches, orbm_projected_point *projected_out,
                                                   orbm_window_query *queries_out, SearchChain *chain)
{
    if (!cur || bad_view(view) || !Tcw || bad_points(points, true, true, false, view->nlevels) || !nmatches || (points->n && !match_q) ||
        (cur->n && !match_kp))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(cur)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    PointsPrefix px;
    px.pts = points; px.scale = view->scale_factors; px.frustum = true; px.proj_host = projected_out;
    px.cam.nlevels = view->nlevels;
    ProjectCam &pc = px.pcam;
    pc.fx = view->fx; pc.fy = view->fy; pc.cx = view->cx; pc.cy = view->cy;
    pc.min_x = cur->min_x; pc.max_x = cur->max_x; pc.min_y = cur->min_y; pc.max_y = cur->max_y;
    pc.mbf = view->mbf; pc.cos_limit = viewing_cos_limit; pc.log_scale = view->log_scale_factor; pc.th = th;
    pose_parts(Tcw, pc.R, pc.t);
    neg_Rt_t(pc.R, pc.t, pc.Ow);                 // mOw = -mRcw.t() * mtcw (Frame::UpdatePoseMatrices, src/Frame.cc:236-242)
    pc.nlevels = view->nlevels; pc.mode = ORBM_PROJECT_FRUSTUM;
    if (projected_out) for (int i = 0; i < points->n; ++i) projected_out[i] = {0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
    FrameSrc fs(cur);
    SeqSearch r;
    r.prefix = &px; r.q.desc = points->desc; r.qtakes = points->takes; r.nq = points->n;
    r.fs = &fs; r.n = cur->n; r.occupied = occupied; r.has_uright = cur->has_uright;
    r.th = th_high; r.nnratio = nnratio; r.accept_mode = ACCEPT_RATIO_SAME_LEVEL;
    r.match_kp = match_kp; r.match_q = match_q; r.nmatches = nmatches; r.queries_out = reinterpret_cast<WinQuery *>(queries_out);
    r.chain = chain;
    return run_sequential(r);
}

int orbm_detail::search_by_projection_last_chain(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const float *Tlw,
                                                 const orbm_points *last, const uint8_t *occupied, float th, int mono, int th_high,
                                                 int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches,
                                                 orbm_window_query *queries_out, SearchChain *chain)
{
    if (!cur || bad_view(view) || !Tcw || !Tlw || bad_points(last, false, false, true, view->nlevels) || !nmatches ||
        (last->n && !match_q) || (cur->n && !match_kp) || (check_orientation && last->n && !last->angle))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(cur)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    PointsPrefix px;
    px.pts = last; px.scale = view->scale_factors;
    form_cam_common(px.cam, view, cur, FORM_LAST, th);
    float Rlw[9], tlw[3], twc[3], tlc[3];
    pose_parts(Tcw, px.cam.R, px.cam.t);                    // Rcw, tcw (:1539-1540)
    pose_parts(Tlw, Rlw, tlw);
    neg_Rt_t(px.cam.R, px.cam.t, twc);                      // twc = -Rcw.t() * tcw (:1542)
    gemm3(Rlw, twc, 1.0, tlw, 1.0, tlc);                    // tlc = Rlw * twc + tlw (:1547)
    px.cam.forward = tlc[2] > view->mb && !mono;            // :1549-1550
    px.cam.backward = -tlc[2] > view->mb && !mono;
    FrameSrc fs(cur);
    SeqSearch r;
    r.prefix = &px; r.q.desc = last->desc; r.q.angle = last->angle; r.qtakes = last->takes; r.nq = last->n;
    r.fs = &fs; r.n = cur->n; r.occupied = occupied; r.has_uright = cur->has_uright;
    r.th = th_high; r.check = check_orientation;
    r.match_kp = match_kp; r.match_q = match_q; r.nmatches = nmatches; r.queries_out = reinterpret_cast<WinQuery *>(queries_out);
    r.chain = chain;
    return run_sequential(r);
}

extern "C" {

int orbm_search_by_projection_last(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const float *Tlw, const orbm_points *last,
                                   const uint8_t *occupied, float th, int mono, int th_high, int check_orientation, int32_t *match_kp,
                                   int32_t *match_q, int *nmatches, orbm_window_query *queries_out)
{
    return search_by_projection_last_chain(cur, view, Tcw, Tlw, last, occupied, th, mono, th_high, check_orientation, match_kp, match_q,
                                           nmatches, queries_out, nullptr);
}

int orbm_search_by_projection_keyframe(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *kf,
                                       const uint8_t *occupied, float th, int orb_dist, int check_orientation, int32_t *match_kp,
                                       int32_t *match_q, int *nmatches, orbm_window_query *queries_out)
{
    if (!cur || bad_view(view) || !Tcw || bad_points(kf, true, false, false, view->nlevels) || !nmatches || (kf->n && !match_q) ||
        (cur->n && !match_kp) || (check_orientation && kf->n && !kf->angle))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(cur)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    PointsPrefix px;
    px.pts = kf; px.scale = view->scale_factors;
    form_cam_common(px.cam, view, cur, FORM_KF, th);
    pose_parts(Tcw, px.cam.R, px.cam.t);
    neg_Rt_t(px.cam.R, px.cam.t, px.cam.Ow);                // Ow = -Rcw.t() * tcw (:1679)
    FrameSrc fs(cur);
    SeqSearch r;     // no stereo test in this form, every assignment blocks its slot (:1741-1742)
    r.prefix = &px; r.q.desc = kf->desc; r.q.angle = kf->angle; r.nq = kf->n;
    r.fs = &fs; r.n = cur->n; r.occupied = occupied;
    r.th = orb_dist; r.check = check_orientation;
    r.match_kp = match_kp; r.match_q = match_q; r.nmatches = nmatches; r.queries_out = reinterpret_cast<WinQuery *>(queries_out);
    return run_sequential(r);
}

int orbm_search_by_projection_sim3(const orbm_frame *kf, const orbm_view *view, const float *Scw, const orbm_points *points,
                                   const uint8_t *occupied, int th, int th_low, int32_t *match_kp, int32_t *match_q, int *nmatches,
                                   orbm_window_query *queries_out)
{
    if (!kf || bad_view(view) || !Scw || bad_points(points, true, true, false, view->nlevels) || !nmatches || (points->n && !match_q) ||
        (kf->n && !match_kp))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(kf)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    PointsPrefix px;
    px.pts = points; px.scale = view->scale_factors;
    form_cam_common(px.cam, view, kf, FORM_SIM3, (float)th);
    {   // :499-504: sRcw, scw = sqrt(sRcw.row(0).dot(sRcw.row(0))), Rcw = sRcw / scw, tcw = Scw.col(3) / scw, Ow = -Rcw.t() * tcw
        float sR[9], st[3];
        pose_parts(Scw, sR, st);
        double dot = 0;
        for (int k = 0; k < 3; ++k) dot += (double)sR[k] * (double)sR[k];
        const float scw = (float)sqrt(dot);
        scale_mat(sR, 9, 1. / scw, px.cam.R);
        scale_mat(st, 3, 1. / scw, px.cam.t);
        neg_Rt_t(px.cam.R, px.cam.t, px.cam.Ow);
    }
    FrameSrc fs(kf);
    SeqSearch r;
    r.prefix = &px; r.q.desc = points->desc; r.nq = points->n;
    r.fs = &fs; r.n = kf->n; r.occupied = occupied;
    r.th = th_low;
    r.match_kp = match_kp; r.match_q = match_q; r.nmatches = nmatches; r.queries_out = reinterpret_cast<WinQuery *>(queries_out);
    return run_sequential(r);
}

int orbm_search_by_sim3(const orbm_frame *kf1, const orbm_frame *kf2, const orbm_view *view, const float *T1w, const float *T2w, float s12,
                        const float *R12, const float *t12, const orbm_points *points1, const orbm_points *points2, float th, int th_high,
                        int32_t *vnMatch1, int32_t *vnMatch2, int32_t *match12, int *nfound, orbm_window_query *q12_out,
                        orbm_window_query *q21_out)
{
    if (!kf1 || !kf2 || bad_view(view) || !T1w || !T2w || !R12 || !t12 || bad_points(points1, true, false, false, view->nlevels) ||
        bad_points(points2, true, false, false, view->nlevels) || !nfound || points1->n != kf1->n || points2->n != kf2->n ||
        (kf1->n && !match12))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(kf1) || bad_octaves(kf2)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    const int n1 = kf1->n, n2 = kf2->n;
    for (int i = 0; i < n1; ++i) { match12[i] = -1; if (vnMatch1) vnMatch1[i] = -1; }
    for (int i = 0; i < n2 && vnMatch2; ++i) vnMatch2[i] = -1;
    *nfound = 0;
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    PointsPrefix p12, p21;
    p12.pts = points1; p21.pts = points2; p12.scale = p21.scale = view->scale_factors;
    form_pair_cams(p12.cam, p21.cam, view, kf1, kf2, T1w, T2w, s12, R12, t12, th);
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    const size_t o_a1 = w.carve((size_t)32 * n1), o_a2 = w.carve((size_t)32 * n2);
    const size_t staged = w.used;
    p12.carve(w); p21.carve(w);                    // read by the prefix kernels from the pinned block
    const size_t pin_in = w.used;
    const size_t o_q12 = w.carve(sizeof(WinQuery) * n1), o_q21 = w.carve(sizeof(WinQuery) * n2), o_b1 = w.carve(sizeof(int) * 5 * (size_t)n1),
                 o_b2 = w.carve(sizeof(int) * 5 * (size_t)n2);
    const size_t o_res = w.used;
    const size_t o_v1 = w.carve(sizeof(int) * n1), o_v2 = w.carve(sizeof(int) * n2), o_m = w.carve(sizeof(int) * n1), o_nf = w.carve(sizeof(int));
    const size_t o_qo1 = w.carve(q12_out ? sizeof(WinQuery) * n1 : 1), o_qo2 = w.carve(q21_out ? sizeof(WinQuery) * n2 : 1);
    const size_t res_bytes = w.used - o_res;
    if (w.reserve(w.used, std::max(pin_in, res_bytes))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    p12.fill(w); p21.fill(w);
    memcpy(w.h<char>(o_a1), points1->desc, (size_t)32 * n1);
    memcpy(w.h<char>(o_a2), points2->desc, (size_t)32 * n2);
    hipStream_t st = w.st;
    ORBX_HIP(hipMemsetAsync(w.d<char>(o_nf), 0, sizeof(int), st));
    if (orbx::stage_ok(w.dev, w.pin, staged)) p12.launch(w, w.d<WinQuery>(o_q12), st, stage_job(w.dev, w.pin, staged));
    else { ORBX_HIP(orbx::stage_in(w.dev, w.pin, staged, st)); p12.launch(w, w.d<WinQuery>(o_q12), st); }
    p21.launch(w, w.d<WinQuery>(o_q21), st);
    FrameSrc f1(kf1), f2(kf2);
    int *b1 = w.d<int>(o_b1), *b2 = w.d<int>(o_b2);
    launch_win_best(st, w.d<WinQuery>(o_q12), w.d<uint4>(o_a1), n1, f2.view(w), nullptr, 0, INT_MAX, nullptr, 0, b1);
    launch_win_best(st, w.d<WinQuery>(o_q21), w.d<uint4>(o_a2), n2, f1.view(w), nullptr, 0, INT_MAX, nullptr, 0, b2);
    hipLaunchKernelGGL(k_sim3_agree, dim3((std::max(n1, n2) + MT - 1) / MT), dim3(MT), 0, st, (const int *)b1, (const int *)(b1 + 4 * n1), n1,
                       (const int *)b2, (const int *)(b2 + 4 * n2), n2, th_high, w.d<int>(o_v1), w.d<int>(o_v2), w.d<int>(o_m), w.d<int>(o_nf));
    ORBX_HIP(hipGetLastError());
    if (q12_out) ORBX_HIP(hipMemcpyAsync(w.d<char>(o_qo1), w.d<char>(o_q12), sizeof(WinQuery) * n1, hipMemcpyDeviceToDevice, st));
    if (q21_out) ORBX_HIP(hipMemcpyAsync(w.d<char>(o_qo2), w.d<char>(o_q21), sizeof(WinQuery) * n2, hipMemcpyDeviceToDevice, st));
    ORBX_HIP(orbx::stage_out(w.pin, w.dev + o_res, res_bytes, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (vnMatch1) memcpy(vnMatch1, w.pin + (o_v1 - o_res), sizeof(int) * n1);
    if (vnMatch2) memcpy(vnMatch2, w.pin + (o_v2 - o_res), sizeof(int) * n2);
    memcpy(match12, w.pin + (o_m - o_res), sizeof(int) * n1);
    memcpy(nfound, w.pin + (o_nf - o_res), sizeof(int));
    if (q12_out) memcpy(q12_out, w.pin + (o_qo1 - o_res), sizeof(WinQuery) * n1);
    if (q21_out) memcpy(q21_out, w.pin + (o_qo2 - o_res), sizeof(WinQuery) * n2);
    return ORBX_OK;
}

} // extern "C"

void orbm_detail::launch_project_pair_jobs(hipStream_t st, const PairSearchJob *djobs, int njobs, int max_nq, char *ws, const float *dscale)
{
    hipLaunchKernelGGL(k_project_pair_jobs, dim3((max_nq + MT - 1) / MT, njobs), dim3(MT), 0, st, djobs, ws, dscale);
}
