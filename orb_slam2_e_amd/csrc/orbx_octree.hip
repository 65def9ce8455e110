// orbx_octree.hip -- DistributeOctTree (ORBextractor.cc:539-763) as scan-based rounds: k_octree, one workgroup per (level, frame),
// in a 256-thread and a 512-thread instantiation.  The host side below it sizes the node pool, the key slots and the ranking key
// (plan_octree), raises the LDS limit of both instantiations (prepare_octree) and chooses between them by batch size (launch_octree).
#include <stdlib.h>

#include <algorithm>

#include "orbx_extract_internal.h"

using namespace orbx_detail;

ORBX_PHASE_UNIT(octree)

namespace {

// ------------------------------------------------------------------- octree
// Exclusive scan of a[0..n) (and, if b != nullptr, of b[0..n)) in place by the
// whole 256-thread block; totals returned through ta / tb.  Each thread owns a
// contiguous chunk, wave-level shuffle scan, one cross-wave hop through LDS:
// three barriers in all.
template <int T>
__device__ void block_excl_scan2(int *a, int *b, int n, int *part, int &ta, int &tb)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __syncthreads();
    const int per = (n + T - 1) / T;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int sa = 0, sb = 0;
    for (int i = lo; i < hi; ++i) { sa += a[i]; if (b) sb += b[i]; }
    // inclusive over the wave (this kernel is a chain of ~20 such scans, each waited for)
    const int ia = orbx::wave_incl_scan(sa), ib = b ? orbx::wave_incl_scan(sb) : 0;
    if (lane == 63) { part[w] = ia; part[T / 64 + w] = ib; }
    __syncthreads();
    int ba = 0, bb = 0, ga = 0, gb = 0;
#pragma unroll
    for (int i = 0; i < T / 64; ++i) {
        if (i < w) { ba += part[i]; bb += part[T / 64 + i]; }
        ga += part[i]; gb += part[T / 64 + i];
    }
    int ra = ba + ia - sa, rb = bb + ib - sb;
    for (int i = lo; i < hi; ++i) {
        const int va = a[i];
        a[i] = ra; ra += va;
        if (b) { const int vb = b[i]; b[i] = rb; rb += vb; }
    }
    ta = ga; tb = gb;
    __syncthreads();
}
template <int T>
__device__ int block_excl_scan(int *a, int n, int *part)
{
    int ta, tb;
    block_excl_scan2<T>(a, nullptr, n, part, ta, tb);
    return ta;
}

// Children of node box (x0,x1,y0,y1): ExtractorNode::DivideNode, ORBextractor.cc:481-509.
__device__ __forceinline__ void child_box(int x0, int x1, int y0, int y1, int q, int &cx0, int &cx1, int &cy0, int &cy1)
{
    const int mx = x0 + (int)ceilf((float)(x1 - x0) / 2);
    const int my = y0 + (int)ceilf((float)(y1 - y0) / 2);
    cx0 = (q & 1) ? mx : x0;
    cx1 = (q & 1) ? x1 : mx;
    cy0 = (q & 2) ? my : y0;
    cy1 = (q & 2) ? y1 : my;
}

// DistributeOctTree (ORBextractor.cc:539-763) for one (level, frame) per block.
// Each pass of the reference's list surgery is one "round": which nodes split,
// where their children land in the list, and where the untouched nodes move are
// all prefix sums (tests/octree_model.py is the same formulation in Python and is
// checked against the literal list-based oracle).  Equal-size ties in the
// largest-first phase use creation order.
// Keys (candidates) live in LDS when the level has at most `kcap` of them, else in
// the per-frame HBM workspace (flat pointers serve both).
template <int T, int KPT, int KB>
__global__ __launch_bounds__(T) void k_octree(const LevelInfo *__restrict__ L, const CellInfo *__restrict__ cells,
                                                  const int *__restrict__ cell_count, int cells_per_frame,
                                                  const uint32_t *__restrict__ cands, size_t cands_per_frame,
                                                  uint32_t *__restrict__ kpos_all, unsigned short *__restrict__ knode_all,
                                                  uint8_t *__restrict__ kq_all, size_t keys_per_frame,
                                                  uint32_t *__restrict__ sel_all, int sel_per_frame,
                                                  int *__restrict__ level_count, int *__restrict__ level_ncand,
                                                  int nlevels, int NC, int maxcells, int kcap, int kshift)
{
    extern __shared__ __align__(16) unsigned char smem[];
    int *p = reinterpret_cast<int *>(smem);
    int *part = p;          p += 2 * (T / 64);
    int *s_cell = p;        p += (maxcells + 1 + 3) & ~3;
    int *s_coff = p;        p += (maxcells + 1 + 3) & ~3; // each cell's slot in the candidate buffer
    int *bx[2] = {p, p + NC};  p += 2 * NC; // x0 | x1<<16
    int *by[2] = {p, p + NC};  p += 2 * NC; // y0 | y1<<16
    int *cnt[2] = {p, p + NC}; p += 2 * NC;
    // narrow per-node fields share dwords (NC is a multiple of 4): 16 NC dwords of node state in all
    unsigned short *seq[2] = {reinterpret_cast<unsigned short *>(p), reinterpret_cast<unsigned short *>(p) + NC}; p += NC; // < NC
    int *cc = p;            p += 4 * NC;
    uint8_t *nne = reinterpret_cast<uint8_t *>(p), *eexp = nne + NC, *split = nne + 2 * NC; p += NC; // 0..4, 0..4, flag
    unsigned short *order = reinterpret_cast<unsigned short *>(p), *bstart = order + NC;      p += NC; // node / list positions
    int *ebase = p;         p += NC;
    int *a1 = p;            p += NC;
    int *a2 = p;            p += NC;
    uint32_t *l_kpos = reinterpret_cast<uint32_t *>(p);                     p += kcap;
    unsigned short *l_knode = reinterpret_cast<unsigned short *>(p);        p += (kcap + 1) / 2;
    uint8_t *l_kq = reinterpret_cast<uint8_t *>(p);
    __shared__ int s_nproc;

    const int l = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    ORBX_PH_INIT(3);
#ifdef ORBX_PHASE_TIMING
    if (tid == 0) { for (int i = 0; i < 8; ++i) ph_rec[i] = 0; ph_rec[12] = l; }
#endif
    const LevelInfo lv = L[l];
    const int N = lv.N;

    // gather the level's candidates in cell row-major order (vToDistributeKeys)
    // (cand_off goes to LDS too, so that the gather below has one dependent global load per candidate, not two)
    for (int c = tid; c < lv.ncells; c += T) {
        const int n = cell_count[(size_t)f * cells_per_frame + lv.cell_base + c];
        const CellInfo ci = cells[lv.cell_base + c];
        s_cell[c] = n < ci.cap ? n : ci.cap;
        s_coff[c] = ci.cand_off;
    }
    const int M = block_excl_scan<T>(s_cell, lv.ncells, part);
    if (tid == 0) s_cell[lv.ncells] = M;
    const bool in_lds = M <= kcap;
    uint32_t *kpos = in_lds ? l_kpos : kpos_all + (size_t)f * keys_per_frame + lv.key_base;
    unsigned short *knode = in_lds ? l_knode : knode_all + (size_t)f * keys_per_frame + lv.key_base;
    uint8_t *kq = in_lds ? l_kq : kq_all + (size_t)f * keys_per_frame + lv.key_base;
    uint32_t *kpos_out = kpos_all + (size_t)f * keys_per_frame + lv.key_base; // candidates stay readable for staged tests
    for (int i = tid; i < NC; i += T) cnt[0][i] = 0;
    __syncthreads();
    // Up to KPT x 256 candidates (every level of a usual frame) the keys never leave the registers: thread t owns the keys
    // t, t + 256, ...; a key's packed position never changes and its node is rewritten by its owner only.  A round's two passes
    // over the keys were 60 % of a workgroup's life as loops over LDS / HBM arrays -- every iteration a chain of dependent
    // reads (node of the key -> state of the node) on a workgroup of four waves; with the keys in registers all of a thread's
    // node-state reads are in flight together.
    const bool regs = M <= KPT * T;
    uint32_t kp[KPT];
    int kn[KPT], kqv[KPT];
    if (regs) {
        // cell of key k = largest c with s_cell[c] <= k: the bisections of a thread's keys run in lockstep, one LDS read of each
        // in flight per step (one after the other they were 8 x 9 dependent reads)
        // (KB keys at a time here and in the passes below: batching all eight took 187 VGPRs, and what the kernel holds on
        // a CU for 60 us is what the other contexts' kernels cannot have -- the step lost 4 % to it)
#pragma unroll
        for (int u = 0; u < KPT; ++u) { kp[u] = 0; kn[u] = 0; kqv[u] = 0; }
#pragma unroll
        for (int h = 0; h < KPT; h += KB) {
            if (h * T >= M) break;
            int lo[KB], hi[KB];
#pragma unroll
            for (int v = 0; v < KB; ++v) { lo[v] = 0; hi[v] = lv.ncells; }
            for (int span = lv.ncells; span > 1; span = (span + 1) >> 1) {
#pragma unroll
                for (int v = 0; v < KB; ++v) {
                    const int mid = (lo[v] + hi[v]) >> 1;
                    if (hi[v] - lo[v] > 1) { if (s_cell[mid] <= min(tid + (h + v) * T, M - 1)) lo[v] = mid; else hi[v] = mid; }
                }
            }
#pragma unroll
            for (int v = 0; v < KB; ++v) {
                const int k = tid + (h + v) * T;
                if (k < M) kp[h + v] = cands[(size_t)f * cands_per_frame + s_coff[lo[v]] + (k - s_cell[lo[v]])];
            }
        }
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const int k = tid + u * T;
            if (k < M) {
                kpos_out[k] = kp[u];
                const float x = (float)((kp[u] >> 8) & 0xfffu);
                kn[u] = (int)(x / lv.hX); // vpIniNodes[kp.pt.x/hX], :569
                atomicAdd(&cnt[0][kn[u]], 1);
            }
        }
    } else
    for (int k0 = tid; k0 < M; k0 += 4 * T) { // four candidates per thread in flight: the loads are a dependent chain each
        uint32_t pk4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * T;
            pk4[u] = 0;
            if (k < M) {
                int lo = 0, hiC = lv.ncells; // largest c with s_cell[c] <= k
                while (hiC - lo > 1) {
                    const int mid = (lo + hiC) >> 1;
                    if (s_cell[mid] <= k) lo = mid; else hiC = mid;
                }
                pk4[u] = cands[(size_t)f * cands_per_frame + s_coff[lo] + (k - s_cell[lo])];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * T;
            if (k < M) {
                const uint32_t pk = pk4[u];
                kpos[k] = pk;
                if (in_lds) kpos_out[k] = pk;
                const float x = (float)((pk >> 8) & 0xfffu);
                const int root = (int)(x / lv.hX); // vpIniNodes[kp.pt.x/hX], :569
                knode[k] = (unsigned short)root;
                atomicAdd(&cnt[0][root], 1);
            }
        }
    }
    __syncthreads();
    ORBX_PHA(0, tid == 0);   // cells, scan, candidate gather
#ifdef ORBX_PHASE_TIMING
    if (tid == 0) ph_rec[11] = M;
#endif
    // roots (:552-563), empty ones erased (:574-585)
    for (int i = tid; i < lv.nIni; i += T) a1[i] = cnt[0][i] > 0 ? 1 : 0;
    int S = block_excl_scan<T>(a1, lv.nIni, part);
    for (int i = tid; i < lv.nIni; i += T) {
        if (cnt[0][i] > 0) {
            const int x0 = (int)(lv.hX * (float)i), x1 = (int)(lv.hX * (float)(i + 1));
            const int pos = a1[i];
            bx[1][pos] = x0 | (x1 << 16);
            by[1][pos] = 0 | (lv.H << 16);
            cnt[1][pos] = cnt[0][i];
            seq[1][pos] = 0;
        }
    }
    if (regs) {
#pragma unroll
        for (int u = 0; u < KPT; ++u) { if (u * T >= M) break; kn[u] = tid + u * T < M ? a1[kn[u]] : 0; }
    } else
    for (int k = tid; k < M; k += T) knode[k] = (unsigned short)a1[knode[k]];
    __syncthreads();
    ORBX_PHA(1, tid == 0);   // roots
    int cur = 1, mode = 1;

    while (true) {
        int *cx = bx[cur], *cy = by[cur], *cn = cnt[cur];
        unsigned short *cs = seq[cur];
        for (int s = tid; s < S; s += T) {
            cc[4 * s] = cc[4 * s + 1] = cc[4 * s + 2] = cc[4 * s + 3] = 0;
            split[s] = 0;
        }
        __syncthreads();
        // children counts of every expandable node (DivideNode, :511-526)
        if (regs) {
#pragma unroll
            for (int h = 0; h < KPT; h += KB) {
                if (h * T >= M) break;
                int ncn[KB], ncx[KB], ncy[KB];   // the node's state, read for KB of the thread's keys at once
#pragma unroll
                for (int v = 0; v < KB; ++v) { ncn[v] = cn[kn[h + v]]; ncx[v] = cx[kn[h + v]]; ncy[v] = cy[kn[h + v]]; }
#pragma unroll
                for (int v = 0; v < KB; ++v) {
                    const int u = h + v;
                    if (tid + u * T < M && ncn[v] > 1) {
                        const float x = (float)((kp[u] >> 8) & 0xfffu), y = (float)(kp[u] >> 20);
                        const int x0 = ncx[v] & 0xffff, x1 = ncx[v] >> 16, y0 = ncy[v] & 0xffff, y1 = ncy[v] >> 16;
                        const int mx = x0 + (int)ceilf((float)(x1 - x0) / 2);
                        const int my = y0 + (int)ceilf((float)(y1 - y0) / 2);
                        kqv[u] = (x < (float)mx ? 0 : 1) + (y < (float)my ? 0 : 2);
                        atomicAdd(&cc[4 * kn[u] + kqv[u]], 1);
                    }
                }
            }
        } else
        for (int k = tid; k < M; k += T) {
            const int s = knode[k];
            if (cn[s] > 1) {
                const uint32_t pk = kpos[k];
                const float x = (float)((pk >> 8) & 0xfffu), y = (float)(pk >> 20);
                const int x0 = cx[s] & 0xffff, x1 = cx[s] >> 16, y0 = cy[s] & 0xffff, y1 = cy[s] >> 16;
                const int mx = x0 + (int)ceilf((float)(x1 - x0) / 2);
                const int my = y0 + (int)ceilf((float)(y1 - y0) / 2);
                const int q = (x < (float)mx ? 0 : 1) + (y < (float)my ? 0 : 2);
                kq[k] = (uint8_t)q;
                atomicAdd(&cc[4 * s + q], 1);
            }
        }
        __syncthreads();
        ORBX_PHA(2, tid == 0);   // children counts (pass over the keys)
        // per node: non-empty / expandable children; scanned together with the candidate flag
        for (int s = tid; s < S; s += T) {
            int a = 0, b = 0;
            const bool cand = cn[s] > 1;
            if (cand) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a += cc[4 * s + q] > 0;
                    b += cc[4 * s + q] > 1;
                }
            }
            nne[s] = a;
            eexp[s] = b;
            a1[s] = cand ? 1 : 0;      // -> candidate index in list order
            a2[s] = a | (b << 16);     // -> prefix of (non-empty, expandable) children in list order
        }
        int E, PE;
        block_excl_scan2<T>(a1, a2, S, part, E, PE);
        ORBX_PHA(3, tid == 0);   // node flags + scans
        if (E == 0) break;
        int F, Etot, nns;
        if (mode == 1) {
            // every expandable node splits, in list order (:606-665)
            F = PE & 0xffff; Etot = PE >> 16;
            for (int s = tid; s < S; s += T) {
                if (cn[s] > 1) {
                    split[s] = 1;
                    bstart[s] = F - ((a2[s] & 0xffff) + nne[s]); // children pushed to the front, last processed first
                    ebase[s] = a2[s] >> 16;
                }
                a1[s] = s - a1[s]; // rank among the nodes that stay
            }
            nns = S - E;
            __syncthreads();
        } else {
            // largest first, later-created first among equals (:684-732): rank = number of expandable nodes with a
            // larger (size, creation seq) key.  Keys (size << kshift | seq, seq < NC <= 2^kshift; 0 for the others) are packed first so that
            // the S x S comparison reads one LDS dword per four nodes (it was 45 % of the kernel as a scalar loop).
            unsigned *okey = reinterpret_cast<unsigned *>(ebase); // free until the splits are numbered below
            if (kshift) {
                for (int s = tid; s < ((S + 3) & ~3); s += T) okey[s] = (s < S && cn[s] > 1) ? ((unsigned)cn[s] << kshift) | cs[s] : 0u;
                __syncthreads();
                for (int s = tid; s < S; s += T) {
                    const unsigned k0 = okey[s];
                    if (k0) {
                        int r = 0;
                        for (int s2 = 0; s2 < S; s2 += 4) {
                            const uint4 k4 = *reinterpret_cast<const uint4 *>(okey + s2);
                            r += (k4.x > k0) + (k4.y > k0) + (k4.z > k0) + (k4.w > k0);
                        }
                        order[r] = (unsigned short)s;
                    }
                }
            } else {
                // a level with 2^21 candidate slots or more (frames beyond ~8 M pixels): size and sequence do not fit one dword,
                // the pairs are compared as they are (the plain loop the packed keys replaced: slower, exact)
                for (int s = tid; s < S; s += T) {
                    const int c0 = cn[s], q0 = cs[s];
                    if (c0 > 1) {
                        int r = 0;
                        for (int s2 = 0; s2 < S; ++s2) {
                            const int c2 = cn[s2];
                            r += c2 > 1 && (c2 > c0 || (c2 == c0 && (int)cs[s2] > q0));
                        }
                        order[r] = (unsigned short)s;
                    }
                }
            }
            __syncthreads(); // okey (= ebase) is rewritten below
            if (tid == 0) s_nproc = E;
            __syncthreads();
            for (int r = tid; r < E; r += T) a2[r] = nne[order[r]] | (eexp[order[r]] << 16);
            int dummy;
            block_excl_scan2<T>(a2, nullptr, E, part, PE, dummy);
            for (int r = tid; r < E; r += T) // stop at the first split that reaches N leaves (:730-731)
                if (S + (a2[r] & 0xffff) - r + nne[order[r]] - 1 >= N) atomicMin(&s_nproc, r + 1);
            __syncthreads();
            const int nproc = s_nproc;
            // totals over the processed prefix
            const int lastr = nproc - 1, lasts = order[lastr];
            F = (a2[lastr] & 0xffff) + nne[lasts];
            Etot = (a2[lastr] >> 16) + eexp[lasts];
            for (int r = tid; r < nproc; r += T) {
                const int s = order[r];
                split[s] = 1;
                bstart[s] = F - ((a2[r] & 0xffff) + nne[s]);
                ebase[s] = a2[r] >> 16;
            }
            __syncthreads();
            for (int s = tid; s < S; s += T) a1[s] = split[s] ? 0 : 1;
            nns = block_excl_scan<T>(a1, S, part); // a1[s] = rank among the nodes that stay
        }
        const int S2 = F + nns;
        int *nx = bx[cur ^ 1], *ny = by[cur ^ 1], *nn = cnt[cur ^ 1];
        unsigned short *ns = seq[cur ^ 1];
        ORBX_PHA(4, tid == 0);   // which nodes split (mode 1: all; mode 2: ranking, largest first)
        for (int s = tid; s < S; s += T) {
            if (split[s]) {
                const int x0 = cx[s] & 0xffff, x1 = cx[s] >> 16, y0 = cy[s] & 0xffff, y1 = cy[s] >> 16;
                int e = ebase[s];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = cc[4 * s + q];
                    if (c > 0) {
                        int after = 0;
                        for (int q2 = q + 1; q2 < 4; ++q2) after += cc[4 * s + q2] > 0;
                        const int pos = bstart[s] + after; // list shows n4,n3,n2,n1
                        int c0, c1, d0, d1;
                        child_box(x0, x1, y0, y1, q, c0, c1, d0, d1);
                        nx[pos] = c0 | (c1 << 16);
                        ny[pos] = d0 | (d1 << 16);
                        nn[pos] = c;
                        ns[pos] = c > 1 ? e++ : 0;
                    }
                }
            } else {
                const int pos = F + a1[s];
                nx[pos] = cx[s]; ny[pos] = cy[s]; nn[pos] = cn[s]; ns[pos] = cs[s];
            }
        }
        if (regs) {
#pragma unroll
            for (int h = 0; h < KPT; h += KB) {
                if (h * T >= M) break;
                int nsp[KB], nbs[KB], na1[KB];
                int4 ncc[KB];
#pragma unroll
                for (int v = 0; v < KB; ++v) {
                    const int s = kn[h + v];
                    nsp[v] = split[s]; nbs[v] = bstart[s]; na1[v] = a1[s];
                    ncc[v] = *reinterpret_cast<const int4 *>(cc + 4 * s);
                }
#pragma unroll
                for (int v = 0; v < KB; ++v) {
                    const int u = h + v, q = kqv[u];
                    const int after = (q < 1 && ncc[v].y > 0) + (q < 2 && ncc[v].z > 0) + (q < 3 && ncc[v].w > 0);   // later non-empty children
                    kn[u] = tid + u * T < M ? (nsp[v] ? nbs[v] + after : F + na1[v]) : 0;
                }
            }
        } else
        for (int k = tid; k < M; k += T) {
            const int s = knode[k];
            int pos;
            if (split[s]) {
                const int q = kq[k];
                int after = 0;
                for (int q2 = q + 1; q2 < 4; ++q2) after += cc[4 * s + q2] > 0;
                pos = bstart[s] + after;
            } else {
                pos = F + a1[s];
            }
            knode[k] = (unsigned short)pos;
        }
        __syncthreads();
        ORBX_PHA(5, tid == 0);   // new node list + keys to their new nodes (pass over the keys)
#ifdef ORBX_PHASE_TIMING
        if (tid == 0) ph_rec[7] += 1;
#endif
        const int prevS = S;
        S = S2;
        cur ^= 1;
        if (S >= N || S == prevS) break;          // :669-672, :734-735
        if (mode == 1 && S + 3 * Etot > N) mode = 2; // :673
    }
    __syncthreads();
    // best response per leaf, first candidate wins ties (:741-760)
    int *best = a2;
    for (int s = tid; s < S; s += T) best[s] = 0;
    __syncthreads();
    if (regs) {
#pragma unroll
        for (int u = 0; u < KPT; ++u)
            if (tid + u * T < M)
                atomicMax(reinterpret_cast<unsigned *>(&best[kn[u]]), ((kp[u] & 0xffu) << 24) | (0xffffffu - (unsigned)(tid + u * T)));
    } else
    for (int k = tid; k < M; k += T)
        atomicMax(reinterpret_cast<unsigned *>(&best[knode[k]]), ((kpos[k] & 0xffu) << 24) | (0xffffffu - (unsigned)k));
    __syncthreads();
    uint32_t *sel = sel_all + (size_t)f * sel_per_frame + lv.sel_base;
    const uint32_t *kfin = regs ? kpos_out : kpos;   // (register keys: the gather left the packed positions in the frame's workspace)
    for (int s = tid; s < S; s += T) sel[s] = kfin[0xffffffu - ((unsigned)best[s] & 0xffffffu)];
    if (tid == 0) {
        level_count[f * nlevels + l] = S;
        level_ncand[f * nlevels + l] = M;
    }
    ORBX_PHA(6, tid == 0);   // best response per leaf, output
    ORBX_PH_END(tid == 0);
}

} // namespace

namespace orbx_detail {

// Node pool (NC), key slots in LDS (oct_kcap), the ranking key's shift (oct_kshift) and the LDS budget (oct_lds), from the levels'
// quotas, initial nodes and candidate slots that plan_frame has laid out.
int plan_octree(orbx_extractor *ex)
{
    const int nl = ex->nlevels;
    int maxN = 0;
    for (int l = 0; l < nl; l++) {
        if (ex->lv[l].N > maxN) maxN = ex->lv[l].N;
        if (4 * ex->lv[l].nIni - 4 > maxN) maxN = 4 * ex->lv[l].nIni - 4;   // the first pass leaves up to 4 nIni nodes
    }
    ex->NC = (maxN + 8 + 3) & ~3; // multiple of 4: the node arrays stay 16-byte aligned (int4 reads in k_octree)
    // Keys of a level live in LDS up to this many, else in HBM.  Small on purpose: while k_octree runs (60-80 us of serial
    // rounds) its workgroups pin their LDS on every CU and keep the LDS-hungry kernels of the other pipeline contexts
    // (FAST, blur) off it.  With room for 4096 keys (60 KB per workgroup) the kernel alone is 20 % faster and the
    // 64-frame step 4-5 % slower than with 1536 (39 KB; levels 0-2 of a 640 x 480 frame then keep their keys in HBM).
    // (Since the keys of levels up to 2048 candidates live in registers, the LDS slots only serve larger levels' arrays -- but giving
    // them up (kcap = 0, 28 KB per workgroup) made the step 1 % SLOWER: measured 0.266 against 0.263 ms; kept.)
    ex->oct_kcap = 1536;
    {   // k_octree ranks nodes by size << kshift | creation seq in one dword where that fits (seq < NC <= 2^kshift, kshift = 11 up to
        // a per-level quota of 2,037 features, else 12; a level's candidate slots -- a good quarter of its FAST zone: 3 x 3 strict
        // NMS -- below 2^(32 - kshift)), and by the plain pair otherwise (kshift = 0: frames beyond ~8 M pixels, e.g. 3840 x 2160).
        // What remains a limit: 24 bits for a candidate's index within its level, int offsets per frame.
        size_t worst = 0;
        for (int l = 0; l < nl; l++) {
            const size_t next = l + 1 < nl ? (size_t)ex->lv[l + 1].key_base : ex->keys_per_frame;
            worst = std::max(worst, next - (size_t)ex->lv[l].key_base);
        }
        const int ks = ex->NC <= 2048 ? 11 : 12;
        ex->oct_kshift = worst < ((size_t)1 << (32 - ks)) ? ks : 0;
        if (worst >= ((size_t)1 << 24) || ex->keys_per_frame >= ((size_t)1 << 31) || ex->cands_per_frame >= ((size_t)1 << 31))
            ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 2^24 FAST candidate slots in one pyramid level");
    }
    ex->oct_lds = (int)sizeof(int) * (2 * (OCT_TW / 64) + 2 * ((ex->maxcells + 1 + 3) & ~3) + 16 * ex->NC + ex->oct_kcap + (ex->oct_kcap + 1) / 2 + (ex->oct_kcap + 3) / 4) + 64;
    if (ex->oct_lds > 160 * 1024) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "octree node pool exceeds LDS");
    return ORBX_OK;
}

#define ORBX_OCT_WIDE k_octree<OCT_TW, OCT_KPT * OCT_T / OCT_TW, OCT_KPT * OCT_T / OCT_TW>
#define ORBX_OCT_NARROW k_octree<OCT_T, OCT_KPT, OCT_KB>

int prepare_octree(orbx_extractor *ex)
{
    if (ex->oct_lds > 48 * 1024) {
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ORBX_OCT_NARROW), hipFuncAttributeMaxDynamicSharedMemorySize, ex->oct_lds));
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ORBX_OCT_WIDE), hipFuncAttributeMaxDynamicSharedMemorySize, ex->oct_lds));
    }
    return ORBX_OK;
}

void launch_octree(orbx_extractor *ex, int batch, hipStream_t st)
{
    const int nl = ex->nlevels;
    ex->prof.start(3, st);
    // Small batches: OCT_TW = 512 threads per (level, frame) -- a level's workgroup is the one frame's critical path, and its passes over
    // keys and nodes are loops of dependent LDS reads that twice the threads make half as long: 43.6 -> 37.0 us for one frame (1,024
    // threads: 36.5 -- what is left is the chain of scans and barriers).  Large batches fill the chip with 256-thread workgroups
    // (ORBX_OCT_WIDE_MAX_BATCH moves the limit; tests run both).
    const char *owb = getenv("ORBX_OCT_WIDE_MAX_BATCH");
#define ORBX_OCT_LAUNCH(KERNEL, T_) hipLaunchKernelGGL((KERNEL), dim3(nl, batch), dim3(T_), ex->oct_lds, st, ex->d_lv, ex->d_cells, \
        ex->d_cell_count, ex->cells_per_frame, ex->d_cands, ex->cands_per_frame, ex->d_kpos, \
        ex->d_knode, ex->d_kq, ex->keys_per_frame, ex->d_sel, ex->sel_per_frame, ex->d_level_count, \
        ex->d_level_ncand, nl, ex->NC, ex->maxcells, ex->oct_kcap, ex->oct_kshift)
    if (batch <= (owb ? atoi(owb) : 6)) ORBX_OCT_LAUNCH(ORBX_OCT_WIDE, OCT_TW);
    else ORBX_OCT_LAUNCH(ORBX_OCT_NARROW, OCT_T);
#undef ORBX_OCT_LAUNCH
    ex->prof.stop(3, st);
}

} // namespace orbx_detail
