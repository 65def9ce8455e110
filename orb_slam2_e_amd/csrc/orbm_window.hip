// orbm_window.hip -- window searches whose queries are independent of each other, for gfx950: every query keeps its own best and
// second-best candidate, no query sees what another one matched, so one launch answers them all and nothing is resolved in order.
//   Frame::GetFeaturesInArea                                   src/Frame.cc:342-395
//   the best / second-best loop of SearchByProjection          src/ORBmatcher.cc:69-118     k_win_best (orbm_search_window)
//   the reprojection-error gate of ORBmatcher::Fuse            :1109-1132                   k_win_best, fuse_gate (orbm_search_fuse)
//   the fork's whole-map relocalisation search                 :134-222                     orbm_search_by_projection_map:
//     isInFrustum (:262-330) + ComputeDistance (:224-260)                                     k_map_frustum, k_win_best,
//     TH_RELOC / same-level ratio, last map point wins (:205-216)                             k_reloc_accept
//   that search under every pose PnPsolver::iterate recorded   src/PnPsolver.cc:419-634     k_map_search_poses (..._map_poses),
//     over the caller's arrays or a snapshot of the map in HBM (orbm_map)
//   ORBmatcher::Fuse against every target keyframe             src/ORBmatcher.cc:1053-1150  k_fuse_keyframes (orbm_fuse_keyframes):
//     (LocalMapping.cc:550-558, LoopClosing.cc:587-613)                                       projection + gated walk of all pairs
// The walk over a window's runs of the sorted keypoint array and the selection of the two best are device functions
// (win_best_walk, win_best_select) that k_win_best and k_map_search_poses share; the frustum arithmetic of one map point under one
// pose (map_frustum_point) is shared by k_map_frustum and k_map_search_poses.  A call stages its inputs in the workspace's pinned
// arena, uploads them with one copy, gets its results back in one block and waits for its stream ONCE
// (orbm_debug_last_map_poses_waits).  The frame comes through FrameSrc, on the host or resident (orbm_search_internal.h);
// launch_win_best is also what SearchBySim3 (orbm_search.hip) runs its two directions on.
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "common.h"
#include "orbm_internal.h"
#include "orbm_search_internal.h"
#include "orbx_internal.h"

using namespace orbm_detail;

namespace {

// Window search without coupling between queries = Frame::GetFeaturesInArea (src/Frame.cc:342-395)
// fused with the best / second-best-with-levels loop of SearchByProjection (ORBmatcher.cc:69-118).
// One wave per query walks the window's runs of the sorted keypoint array as k_win_wave does; every
// lane keeps the two smallest keys dist << 16 | position-in-visiting-order of its candidates (strict
// '<', first wins = smallest key; bestDist2 = second smallest), two wave reductions pick the winners.
// Outputs: best / second distance (init_dist when absent), their octaves (-1), arg-best as a
// keypoint index (-1).
// The walk and the selection are device functions (win_best_walk, win_best_select): k_map_search_poses runs the same two on the
// items of its queue.
struct WinBest { unsigned k1, k2, e1, e2; };        // the two smallest keys of a lane and their entries e = octave << 16 | sorted position
struct WinPick { int best, second, blevel, slevel, sp; };   // distances (init_dist when absent), octaves (-1), arg-best as a sorted position (-1)

__device__ __forceinline__ WinBest win_best_walk(const WinQuery &w, const uint4 *__restrict__ a, int lane, const SeqKp *__restrict__ kp,
                                                 const uint4 *__restrict__ B, const int *__restrict__ cell_off,
                                                 const uint8_t *__restrict__ occ, const GridParams &gp, int has_uright, int init_dist,
                                                 const float *__restrict__ inv_sigma2, int fuse_gate)
{
    unsigned k1 = 0xffffffffu, k2 = 0xffffffffu, e1 = 0, e2 = 0; // e = octave << 16 | sorted position
    int c = 0;
    const int nMinCellX = (int)fmaxf(0.f, floorf((w.u - gp.min_x - w.r) * gp.inv_w));
    const int nMaxCellX = (int)fminf((float)FRAME_GRID_COLS - 1, ceilf((w.u - gp.min_x + w.r) * gp.inv_w));
    const int nMinCellY = (int)fmaxf(0.f, floorf((w.v - gp.min_y - w.r) * gp.inv_h));
    const int nMaxCellY = (int)fminf((float)FRAME_GRID_ROWS - 1, ceilf((w.v - gp.min_y + w.r) * gp.inv_h));
    const bool none = !(w.r >= 0.f) || nMinCellX >= FRAME_GRID_COLS || nMaxCellX < 0 || nMinCellY >= FRAME_GRID_ROWS || nMaxCellY < 0;
    if (!none) {
        const bool check_levels = (w.min_level > 0) || (w.max_level >= 0);
        const uint4 a0 = a[0], a1 = a[1];
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            const int r0 = cell_off[ix * FRAME_GRID_ROWS + nMinCellY], r1 = cell_off[ix * FRAME_GRID_ROWS + nMaxCellY + 1];
            for (int kb = r0; kb < r1; kb += 64) {
                const int k = kb + lane;
                bool ok = k < r1;
                SeqKp p = {0.f, 0.f, 0.f, 0};
                if (ok) p = kp[k];
                if (occ && ok) ok = occ[k] == 0;
                if (check_levels) ok = ok && !(p.octave < w.min_level) && !(w.max_level >= 0 && p.octave > w.max_level);
                const float distx = p.x - w.u, disty = p.y - w.v;
                ok = ok && fabsf(distx) < w.r && fabsf(disty) < w.r;
                bool use = ok; // in the visiting order (position) every keypoint of the window counts; `use`: it is scored
                if (fuse_gate == 0) {
                    if (has_uright && p.uright > 0) ok = ok && !(fabsf(w.xr - p.uright) > w.r);
                    use = ok;
                } else if (ok && inv_sigma2) { // reprojection-error gate of ORBmatcher::Fuse (:1109-1132)
                    const float ex = w.u - p.x, ey = w.v - p.y;
                    if (has_uright && p.uright >= 0) {
                        const float er = w.xr - p.uright;
                        const float e2 = ex * ex + ey * ey + er * er;
                        use = !((double)(e2 * inv_sigma2[p.octave]) > 7.8);
                    } else {
                        const float e2 = ex * ex + ey * ey;
                        use = !((double)(e2 * inv_sigma2[p.octave]) > 5.99);
                    }
                }
                const unsigned long long bal = __ballot(ok);
                if (use) {
                    const int dist = popc256(a0, a1, B[2 * k], B[2 * k + 1]);
                    if (dist < init_dist) { // dist<bestDist / dist<bestDist2 can only fire below the initial value
                        const unsigned key = ((unsigned)dist << 16) | (unsigned)(c + __popcll(bal & lt));
                        const unsigned en = ((unsigned)p.octave << 16) | (unsigned)k;
                        if (key < k1) { k2 = k1; e2 = e1; k1 = key; e1 = en; }
                        else if (key < k2) { k2 = key; e2 = en; }
                    }
                }
                c += __popcll(bal);
            }
        }
    }
    return {k1, k2, e1, e2};
}

// smallest key of the wave, then the smallest of what is left (keys are unique); the same result in every lane
__device__ __forceinline__ WinPick win_best_select(const WinBest &t, int init_dist)
{
    const unsigned g1 = wave_min_u32(t.k1);
    const bool own1 = g1 != 0xffffffffu && t.k1 == g1;
    const unsigned long long b1 = __ballot(own1);
    const unsigned c2 = own1 ? t.k2 : t.k1;
    const unsigned g2 = wave_min_u32(c2);
    const unsigned long long b2 = __ballot(g2 != 0xffffffffu && c2 == g2);
    const unsigned w1 = b1 ? (unsigned)__shfl((int)t.e1, __ffsll((long long)b1) - 1) : 0u;
    const unsigned w2 = b2 ? (unsigned)__shfl((int)(own1 ? t.e2 : t.e1), __ffsll((long long)b2) - 1) : 0u;
    WinPick o;
    o.best = b1 ? (int)(g1 >> 16) : init_dist;
    o.sp = b1 ? (int)(w1 & 0xffffu) : -1;
    o.blevel = b1 ? (int)(w1 >> 16) : -1;
    o.second = b2 ? (int)(g2 >> 16) : init_dist;
    o.slevel = b2 ? (int)(w2 >> 16) : -1;
    return o;
}

__global__ __launch_bounds__(MT) void k_win_best(const WinQuery *__restrict__ q, const uint4 *__restrict__ A, int nq,
                                                 const SeqKp *__restrict__ kp, const uint4 *__restrict__ B,
                                                 const int *__restrict__ cell_off, const int *__restrict__ perm, const uint8_t *__restrict__ occ, GridParams gp,
                                                 int has_uright, int init_dist, const float *__restrict__ inv_sigma2, int fuse_gate,
                                                 int *__restrict__ best_o, int *__restrict__ bl_o, int *__restrict__ second_o,
                                                 int *__restrict__ sl_o, int *__restrict__ idx_o)
{
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * (MT / 64) + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (i >= nq) return;
    const WinQuery w = q[i];
    const WinPick o = win_best_select(win_best_walk(w, A + 2 * i, lane, kp, B, cell_off, occ, gp, has_uright, init_dist, inv_sigma2, fuse_gate),
                                      init_dist);
    if (lane == 0) {
        best_o[i] = o.best;
        idx_o[i] = o.sp >= 0 ? perm[o.sp] : -1;
        bl_o[i] = o.blevel;
        second_o[i] = o.second;
        sl_o[i] = o.slevel;
    }
}

// k_win_best as SearchBySim3 runs it (no occupancy, no stereo test, best from INT_MAX) for the jobs of a batch: job blockIdx.y, one
// wave per query.  Only best and idx leave (what the acceptance reads).
__global__ __launch_bounds__(MT) void k_win_best_jobs(const PairSearchJob *__restrict__ jobs, char *__restrict__ ws)
{
    const PairSearchJob &J = jobs[blockIdx.y];
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * (MT / 64) + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (i >= J.nq) return;
    const WinQuery w = reinterpret_cast<const WinQuery *>(ws + J.o_q)[i];
    const WinPick o = win_best_select(win_best_walk(w, reinterpret_cast<const uint4 *>(ws + J.o_desc) + 2 * i, lane, J.frame.kp, J.frame.desc,
                                                    J.frame.cell_off, nullptr, J.frame.gp, 0, INT_MAX, nullptr, 0),
                                      INT_MAX);
    if (lane == 0) {
        reinterpret_cast<int *>(ws + J.o_best)[i] = o.best;
        reinterpret_cast<int *>(ws + J.o_idx)[i] = o.sp >= 0 ? J.frame.perm[o.sp] : -1;
    }
}

// The fork's whole-map relocalisation search (ORBmatcher.cc:134-222): isInFrustum
// (:262-330) + ComputeDistance (:224-260) per map point in the reference's mixed
// float / double arithmetic (fixed op order, no contraction), producing the
// GetFeaturesInArea query of :162-163; k_win_best does the search; then the
// TH_RELOC / same-level ratio acceptance (:205-216) with "last map point wins".
struct MapIntr { float fx, fy, cx, cy; int bminx, bmaxx, bminy, bmaxy; float th; int nlevels; };    // what all poses of a call share
struct MapCam { MapIntr in; double R[9], t[3]; };

// isInFrustum + ComputeDistance + the level and window of one map point under one pose (R, t): the one copy of this arithmetic,
// called by k_map_frustum and k_map_search_poses.  True when the point survives; w and out are written either way.
__device__ __forceinline__ bool map_frustum_point(float ptX, float ptY, float ptZ, float nX, float nY, float nZ, float minDistance,
                                                  float maxDistance, const double *__restrict__ R, const double *__restrict__ t,
                                                  const MapIntr &cam, const float *__restrict__ scale, WinQuery &w, float (&out)[4])
{
    w = {0.f, 0.f, -1.f, 0.f, 0, -1}; // r < 0: no candidates
    out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = -1.f;
    const float PcX = (float)(R[0] * ptX + R[1] * ptY + R[2] * ptZ + t[0]);
    const float PcY = (float)(R[3] * ptX + R[4] * ptY + R[5] * ptZ + t[1]);
    const float PcZ = (float)(R[6] * ptX + R[7] * ptY + R[8] * ptZ + t[2]);
    bool ok = !(PcZ < 0.0f);
    const float invz = (float)(1.0 / (double)PcZ);
    const float u = cam.fx * PcX * invz + cam.cx;
    const float v = cam.fy * PcY * invz + cam.cy;
    ok = ok && !(u < (float)cam.bminx || u > (float)cam.bmaxx) && !(v < (float)cam.bminy || v > (float)cam.bmaxy);
    // ComputeDistance: PO = Pt - (-R^T) t, norm in double
    double PO[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double rtt = ((-1) * R[a]) * t[0] + ((-1) * R[3 + a]) * t[1] + ((-1) * R[6 + a]) * t[2];
        PO[a] = (double)(a == 0 ? ptX : a == 1 ? ptY : ptZ) - rtt;
    }
    const double normSum = PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2];
    const float dist = (float)sqrt(normSum);
    ok = ok && !((double)dist < (0.9 * (double)minDistance) || (double)dist > ((double)maxDistance / 0.9));
    float viewCos = (float)(PO[0] * nX + PO[1] * nY + PO[2] * nZ);
    viewCos = viewCos / dist;
    ok = ok && !(viewCos < 0.5f);
    const float ratio = dist / minDistance;
    int level = 0;
    while (level < cam.nlevels && scale[level] < ratio) ++level; // lower_bound(mvScaleFactors, ratio)
    if (level >= cam.nlevels) level = cam.nlevels - 1;
    if (ok) {
        float r = (double)viewCos > 0.998 ? 3.0f : 4.5f; // RadiusByViewingCos
        if ((double)cam.th != 1.0) r *= cam.th;
        w.u = u; w.v = v; w.r = r * scale[level]; w.min_level = level - 1; w.max_level = level;
        out[0] = u; out[1] = v; out[2] = viewCos; out[3] = (float)level;
    }
    return ok;
}

__global__ __launch_bounds__(MT) void k_map_frustum(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                    const float *__restrict__ mind, const float *__restrict__ maxd, int m,
                                                    MapCam cam, const float *__restrict__ scale, WinQuery *__restrict__ q,
                                                    float *__restrict__ proj)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= m) return;
    WinQuery w;
    float out[4];
    map_frustum_point(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], mind[i], maxd[i], cam.R, cam.t,
                      cam.in, scale, w, out);
    q[i] = w;
    if (proj) { proj[4 * i] = out[0]; proj[4 * i + 1] = out[1]; proj[4 * i + 2] = out[2]; proj[4 * i + 3] = out[3]; }
}

// TH_RELOC and the same-level ratio test (:205-216) on what the window search returned for one map point
__device__ __forceinline__ bool reloc_accepts(int best, int bidx, int second, int blevel, int slevel, int th_reloc, float nnratio)
{
    return bidx >= 0 && best <= th_reloc && !(blevel == slevel && (float)best > nnratio * (float)second);
}

__global__ __launch_bounds__(MT) void k_reloc_accept(const int *__restrict__ best, const int *__restrict__ bidx,
                                                     const int *__restrict__ second, const int *__restrict__ blevel,
                                                     const int *__restrict__ slevel, int m, int th_reloc, float nnratio,
                                                     int *__restrict__ matched, int *__restrict__ nmatches)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    const bool acc = i < m && reloc_accepts(best[i], bidx[i], second[i], blevel[i], slevel[i], th_reloc, nnratio);
    if (acc) atomicMax(&matched[bidx[i]], i); // vMatchedMPs[bestIdx] = pMP: the last map point wins
    const unsigned long long b = __ballot(acc);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(nmatches, __popcll(b));
}

// The whole-map search under P poses in ONE launch (PnPsolver::iterate's second stage, src/PnPsolver.cc:419-634, calls the search
// above once per recorded pose over the same frame and the same map).  A workgroup of MPP_T threads (16 waves) owns MPP_TILE map
// points.  Phase 1: thread (point, pose) of the first MPP_TILE * MPP_MAXP threads does the frustum arithmetic of its pair and
// appends a survivor with its window to a queue in LDS (ballot + popcount per wave, one LDS atomic per wave; MPP_TILE * MPP_MAXP
// entries: it cannot overflow).  Phase 2, behind a barrier: the sixteen waves take the items in turn, one wave per item:
// win_best_walk with the map point's descriptor as the query, win_best_select, reloc_accepts, and lane 0's atomicMax into the
// pose's row of `matched` (the last map point wins, whatever the order).  The acceptances of a pose are counted in LDS and leave
// the workgroup as one atomicAdd per pose.  No query and no best / second array goes through HBM; every loop is bounded by the
// queue length or the window's runs, and no workgroup waits for another.
// A window walk is a chain of dependent loads (cell table -> keypoints -> descriptors) tens of microseconds long, so what decides
// the kernel's time is how many walks a wave does one after the other: 16 points x 16 waves keeps that at P / 4 (a quarter of the
// map survives a pose) with m / 16 workgroups in flight; 64 points x 4 waves made it 4 P with m / 64.
constexpr int MPP_T = 1024, MPP_TILE = 16, MPP_MAXP = 16;
struct MapPose { double R[9], t[3]; };
struct MapItem { float u, v, r; unsigned key; };      // key = point in the tile | pose << 4 | level << 8

__global__ __launch_bounds__(MPP_T) void k_map_search_poses(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                            const float *__restrict__ mind, const float *__restrict__ maxd,
                                                            const uint4 *__restrict__ mdesc, int m, const MapPose *__restrict__ poses, int P,
                                                            MapIntr cam, const float *__restrict__ scale, const SeqKp *__restrict__ kp,
                                                            const uint4 *__restrict__ B, const int *__restrict__ cell_off,
                                                            const int *__restrict__ perm, const uint8_t *__restrict__ occ, GridParams gp, int n,
                                                            int th_reloc, float nnratio, int *__restrict__ matched,
                                                            int *__restrict__ nmatches, float *__restrict__ proj)
{
    __shared__ MapItem s_item[MPP_TILE * MPP_MAXP];
    __shared__ int s_nitems, s_nm[MPP_MAXP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i0 = blockIdx.x * MPP_TILE;
    if (threadIdx.x == 0) s_nitems = 0;
    if (threadIdx.x < MPP_MAXP) s_nm[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < MPP_TILE * MPP_MAXP) {       // (whole waves)
        const int l = threadIdx.x % MPP_TILE, p = threadIdx.x / MPP_TILE, i = i0 + l;
        bool ok = false;
        WinQuery w;
        if (i < m && p < P) {
            float out[4];
            const MapPose &ps = poses[p];
            ok = map_frustum_point(pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1],
                                   nrm[3 * (size_t)i + 2], mind[i], maxd[i], ps.R, ps.t, cam, scale, w, out);
            if (proj) *reinterpret_cast<float4 *>(proj + 4 * ((size_t)p * m + i)) = make_float4(out[0], out[1], out[2], out[3]);
        }
        const unsigned long long bal = __ballot(ok);
        if (bal) {          // (wave-uniform)
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_nitems, __popcll(bal));
            base = __builtin_amdgcn_readfirstlane(base);
            if (ok) s_item[base + __popcll(bal & ((1ull << lane) - 1ull))] = {w.u, w.v, w.r, (unsigned)l | ((unsigned)p << 4) | ((unsigned)w.max_level << 8)};
        }
    }
    __syncthreads();
    const int nitems = s_nitems;        // <= MPP_TILE * P
    for (int it = wave; it < nitems; it += MPP_T / 64) {
        const MapItem e = s_item[it];
        const unsigned key = (unsigned)__builtin_amdgcn_readfirstlane((int)e.key);
        const int i = i0 + (int)(key & 15u), p = (int)((key >> 4) & 15u), level = (int)(key >> 8);
        WinQuery w;
        w.u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.u)));
        w.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.v)));
        w.r = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.r)));
        w.xr = 0.f; w.min_level = level - 1; w.max_level = level;
        const WinPick o = win_best_select(win_best_walk(w, mdesc + 2 * (size_t)i, lane, kp, B, cell_off, occ, gp, 0, INT_MAX, nullptr, 0), INT_MAX);
        if (lane == 0) {
            const int bidx = o.sp >= 0 ? perm[o.sp] : -1;
            if (reloc_accepts(o.best, bidx, o.second, o.blevel, o.slevel, th_reloc, nnratio)) {
                atomicMax(&matched[(size_t)p * n + bidx], i);
                atomicAdd(&s_nm[p], 1);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < P && s_nm[threadIdx.x]) atomicAdd(&nmatches[threadIdx.x], s_nm[threadIdx.x]);
}

// The device half of ORBmatcher::Fuse (projection block src/ORBmatcher.cc:1053-1094 / :1212-1250, gated candidate loop :1092-1150
// / :1252-1277) for every (target keyframe k, list entry i) pair in ONE launch: LocalMapping::SearchInNeighbors and
// LoopClosing::SearchAndFuse call Fuse once per target over the same list.  The grid is (tiles of FK_TILE entries, K): blockIdx.x
// runs fastest, so the workgroups of one target are dispatched together and its cell table and descriptors stay in L2.  The target
// record (frame view, pose, camera) is indexed by blockIdx.y alone: lane-uniform, fetched through scalar loads.
// Phase 1, wave 0: lane l projects entry i0 + l (project_point, the arithmetic k_project_points runs) unless the pair is inactive,
// writes the projected record, and either the rejected result (256, -1) or an item of the LDS queue (ballot + popcount: one wave
// fills it, so no atomic).  Phase 2, behind the barrier: the FK_T / 64 waves take the items in turn, one wave per item:
// win_best_walk with fuse_gate = 1 on target k's frame, win_best_select, lane 0 writes best and idx (through perm).  Most pairs die
// at the mask or in the projection; the walk is a chain of dependent loads (cell table -> keypoints -> descriptors), so what
// decides the time is how many walks a wave does one after the other: at most FK_TILE / (FK_T / 64) = 4.  An inactive pair costs
// one byte read and three preset stores.  Every loop is bounded by the queue length or the window's runs.
constexpr int FK_T = 1024, FK_TILE = 64;
struct FuseTarget { const SeqKp *kp; const uint4 *desc; const int *perm; const int *cell_off; GridParams gp; int has_uright, ns; ProjectCam cam; };
struct FuseItem { float u, v, r, xr; int level, l; };

__global__ __launch_bounds__(FK_T) void k_fuse_keyframes(const FuseTarget *__restrict__ targets, const float *__restrict__ pos,
                                                         const float *__restrict__ nrm, const float *__restrict__ mind,
                                                         const float *__restrict__ maxd, const uint4 *__restrict__ mdesc, int m,
                                                         const uint8_t *__restrict__ active, const float *__restrict__ scale,
                                                         const float *__restrict__ inv_sigma2, int *__restrict__ best_o, int *__restrict__ idx_o,
                                                         orbm_projected_point *__restrict__ proj)
{
    __shared__ FuseItem s_item[FK_TILE];
    __shared__ int s_nitems;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int k = blockIdx.y, i0 = blockIdx.x * FK_TILE;
    const FuseTarget &t = targets[k];
    const size_t row0 = (size_t)k * m;
    if (wave == 0) {
        const int i = i0 + lane;
        bool ok = false;
        WinQuery w;
        if (i < m) {
            orbm_projected_point o = {0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
            if (!active || active[row0 + i]) {
                project_point(i, nullptr, pos, nrm, mind, maxd, t.cam, scale, o, w);
                ok = o.visible && t.ns > 0;     // a keyframe without a keypoint in its grid has no candidate
            }
            if (proj) proj[row0 + i] = o;
            if (!ok) { best_o[row0 + i] = 256; idx_o[row0 + i] = -1; }
        }
        const unsigned long long bal = __ballot(ok);
        if (ok) s_item[__popcll(bal & ((1ull << lane) - 1ull))] = {w.u, w.v, w.r, w.xr, w.max_level, lane};
        if (lane == 0) s_nitems = __popcll(bal);
    }
    __syncthreads();
    const int nitems = s_nitems;        // <= FK_TILE
    for (int it = wave; it < nitems; it += FK_T / 64) {
        const FuseItem e = s_item[it];
        const int level = __builtin_amdgcn_readfirstlane(e.level), i = i0 + __builtin_amdgcn_readfirstlane(e.l);
        WinQuery w;
        w.u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.u)));
        w.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.v)));
        w.r = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.r)));
        w.xr = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e.xr)));
        w.min_level = level - 1; w.max_level = level;
        const WinPick o = win_best_select(win_best_walk(w, mdesc + 2 * (size_t)i, lane, t.kp, t.desc, t.cell_off, nullptr, t.gp, t.has_uright, 256,
                                                        inv_sigma2, 1), 256);
        if (lane == 0) {
            best_o[row0 + i] = o.best;
            idx_o[row0 + i] = o.sp >= 0 ? t.perm[o.sp] : -1;
        }
    }
}

} // namespace

// One window search without coupling (k_win_best) for device-resident queries: returns into ob[5][nq] (best, best level, second,
// second level, idx).
void orbm_detail::launch_win_best(hipStream_t st, const WinQuery *dq, const uint4 *da, int nq, const FrameView &fv, const uint8_t *docc,
                                  int has_uright, int init_dist, const float *inv_sigma2, int fuse_gate, int *ob)
{
    hipLaunchKernelGGL(k_win_best, dim3((nq + MT / 64 - 1) / (MT / 64)), dim3(MT), 0, st, dq, da, nq, fv.kp, fv.desc, fv.cell_off, fv.perm, docc,
                       fv.gp, has_uright, init_dist, inv_sigma2, fuse_gate, ob, ob + nq, ob + 2 * nq, ob + 3 * nq, ob + 4 * nq);
}

void orbm_detail::launch_win_best_jobs(hipStream_t st, const PairSearchJob *djobs, int njobs, int max_nq, char *ws)
{
    hipLaunchKernelGGL(k_win_best_jobs, dim3((max_nq + MT / 64 - 1) / (MT / 64), njobs), dim3(MT), 0, st, djobs, ws);
}

namespace {

int search_window_core(FrameSrc &fs, const orbm_window_query *queries, const uint8_t *qdesc, int nq, const uint8_t *skip, int has_uright,
                       int init_dist, const float *inv_level_sigma2, int nlevels, int fuse_gate, int32_t *best, int32_t *best_level,
                       int32_t *second, int32_t *second_level, int32_t *idx)
{
    const int ns = fs.ns();
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    const size_t o_q = w.carve(sizeof(WinQuery) * nq), o_a = w.carve((size_t)32 * nq);
    fs.carve(w);
    const size_t o_occ = w.carve(skip && ns ? (size_t)ns : 1), o_sg = w.carve(inv_level_sigma2 ? sizeof(float) * nlevels : 1);
    const size_t staged = w.used;
    const size_t o_res = w.carve(sizeof(int) * 5 * (size_t)nq);
    if (w.reserve(w.used, std::max(staged, sizeof(int) * 5 * (size_t)nq + 16))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    memcpy(w.h<char>(o_q), queries, sizeof(WinQuery) * nq);
    memcpy(w.h<char>(o_a), qdesc, (size_t)32 * nq);
    fs.fill(w);
    if (skip && ns) fs.fill_occ(w.h<uint8_t>(o_occ), skip);
    if (inv_level_sigma2) memcpy(w.h<char>(o_sg), inv_level_sigma2, sizeof(float) * nlevels);
    ORBX_HIP(orbx::stage_in(w.dev, w.pin, staged, w.st));
    int *ob = w.d<int>(o_res);
    launch_win_best(w.st, w.d<WinQuery>(o_q), w.d<uint4>(o_a), nq, fs.view(w), skip && ns ? w.d<uint8_t>(o_occ) : nullptr, has_uright, init_dist,
                    inv_level_sigma2 ? w.d<float>(o_sg) : nullptr, fuse_gate, ob);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(orbx::stage_out(w.pin, ob, (sizeof(int) * 5 * (size_t)nq + 15) & ~(size_t)15, w.st));
    ORBX_HIP(hipStreamSynchronize(w.st));
    const int *r = w.h<int>(0);
    if (best) memcpy(best, r, sizeof(int) * nq);
    if (best_level) memcpy(best_level, r + nq, sizeof(int) * nq);
    if (second) memcpy(second, r + 2 * nq, sizeof(int) * nq);
    if (second_level) memcpy(second_level, r + 3 * nq, sizeof(int) * nq);
    if (idx) memcpy(idx, r + 4 * nq, sizeof(int) * nq);
    return ORBX_OK;
}

MapIntr map_intrinsics(const orbm_camera *cam, float th, int nlevels)
{
    return {cam->fx, cam->fy, cam->cx, cam->cy, cam->min_x, cam->max_x, cam->min_y, cam->max_y, th, nlevels};
}

std::atomic<int> g_last_map_poses_waits{0};    // host waits of the last ..._map_poses call of this process
std::atomic<int> g_last_fuse_keyframes_waits{0};    // host waits of the last orbm_fuse_keyframes call of this process

// The map of a whole-map search: the caller's host arrays, staged with the call, or a snapshot's device block (carve and fill then
// do nothing), in the manner of FrameSrc.
struct MapSrc {
    const float *pos, *nrm, *mind, *maxd;
    const uint8_t *desc;
    const orbm_map *snap;
    int m;
    size_t o_pos = 0, o_nrm = 0, o_min = 0, o_max = 0, o_md = 0;
    void carve(Workspace &w)
    {
        if (snap) return;
        o_pos = w.carve(sizeof(float) * 3 * m); o_nrm = w.carve(sizeof(float) * 3 * m); o_min = w.carve(sizeof(float) * m);
        o_max = w.carve(sizeof(float) * m); o_md = w.carve((size_t)32 * m);
    }
    void fill(Workspace &w) const
    {
        if (snap) return;
        memcpy(w.h<char>(o_pos), pos, sizeof(float) * 3 * m); memcpy(w.h<char>(o_nrm), nrm, sizeof(float) * 3 * m);
        memcpy(w.h<char>(o_min), mind, sizeof(float) * m); memcpy(w.h<char>(o_max), maxd, sizeof(float) * m);
        memcpy(w.h<char>(o_md), desc, (size_t)32 * m);
    }
    const float *d_pos(const Workspace &w) const { return snap ? snap->pos : w.d<float>(o_pos); }
    const float *d_nrm(const Workspace &w) const { return snap ? snap->nrm : w.d<float>(o_nrm); }
    const float *d_min(const Workspace &w) const { return snap ? snap->mind : w.d<float>(o_min); }
    const float *d_max(const Workspace &w) const { return snap ? snap->maxd : w.d<float>(o_max); }
    const uint4 *d_desc(const Workspace &w) const { return snap ? snap->desc : w.d<uint4>(o_md); }
};

int search_map_core(FrameSrc &fs, int n, const uint8_t *has_mappoint, MapSrc &map, const double *Rcw, const double *tcw,
                    const orbm_camera *cam, const float *scale_factors, int nlevels, float th, float nnratio, int th_reloc,
                    int32_t *matched_mp, int *nmatches, float *proj)
{
    const int ns = fs.ns(), m = map.m;
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    map.carve(w);
    fs.carve(w);
    const size_t o_occ = w.carve(has_mappoint && ns ? (size_t)ns : 1), o_sc = w.carve(sizeof(float) * nlevels);
    const size_t staged = w.used;
    const size_t o_q = w.carve(sizeof(WinQuery) * m), o_o = w.carve(sizeof(int) * 5 * (size_t)m);
    const size_t o_res = w.used;
    const size_t o_mk = w.carve(sizeof(int) * n), o_nm = w.carve(sizeof(int)), o_proj = w.carve(sizeof(float) * 4 * m);
    const size_t res_bytes = w.used - o_res;
    if (w.reserve(w.used, std::max(staged, res_bytes))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    map.fill(w);
    fs.fill(w);
    if (has_mappoint && ns) fs.fill_occ(w.h<uint8_t>(o_occ), has_mappoint);
    memcpy(w.h<char>(o_sc), scale_factors, sizeof(float) * nlevels);
    hipStream_t st = w.st;
    ORBX_HIP(orbx::stage_in(w.dev, w.pin, staged, st));
    ORBX_HIP(hipMemsetAsync(w.d<char>(o_mk), 0xff, sizeof(int) * n, st));
    ORBX_HIP(hipMemsetAsync(w.d<char>(o_nm), 0, sizeof(int), st));
    MapCam mc;
    mc.in = map_intrinsics(cam, th, nlevels);
    for (int i = 0; i < 9; ++i) mc.R[i] = Rcw[i];
    for (int i = 0; i < 3; ++i) mc.t[i] = tcw[i];
    int *ob = w.d<int>(o_o);
    const dim3 g((m + MT - 1) / MT);
    hipLaunchKernelGGL(k_map_frustum, g, dim3(MT), 0, st, map.d_pos(w), map.d_nrm(w), map.d_min(w), map.d_max(w), m, mc,
                       (const float *)w.d<float>(o_sc), w.d<WinQuery>(o_q), w.d<float>(o_proj));
    launch_win_best(st, w.d<WinQuery>(o_q), map.d_desc(w), m, fs.view(w), has_mappoint && ns ? w.d<uint8_t>(o_occ) : nullptr, 0, INT_MAX,
                    nullptr, 0, ob);
    hipLaunchKernelGGL(k_reloc_accept, g, dim3(MT), 0, st, (const int *)ob, (const int *)(ob + 4 * m), (const int *)(ob + 2 * m),
                       (const int *)(ob + m), (const int *)(ob + 3 * m), m, th_reloc, nnratio, w.d<int>(o_mk), w.d<int>(o_nm));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(orbx::stage_out(w.pin, w.dev + o_res, res_bytes, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(matched_mp, w.pin + (o_mk - o_res), sizeof(int) * n);
    if (nmatches) memcpy(nmatches, w.pin + (o_nm - o_res), sizeof(int));
    if (proj) memcpy(proj, w.pin + (o_proj - o_res), sizeof(float) * 4 * m);
    return ORBX_OK;
}

// One upload (the map and the frame only where they are host arrays; has_mappoint by sorted position, the poses, the scale
// factors), the presets, k_map_search_poses, one result block, one wait.
int search_map_poses_core(FrameSrc &fs, int n, const uint8_t *has_mappoint, MapSrc &map, const double *Rcw, const double *tcw, int P,
                          const orbm_camera *cam, const float *scale_factors, int nlevels, float th, float nnratio, int th_reloc,
                          int32_t *matched_mp, int32_t *nmatches, float *proj)
{
    const int ns = fs.ns(), m = map.m;
    WorkspaceLease lease;
    Workspace &w = *lease.w;
    w.used = 0;
    map.carve(w);
    fs.carve(w);
    const size_t o_occ = w.carve(has_mappoint && ns ? (size_t)ns : 1), o_pose = w.carve(sizeof(MapPose) * P), o_sc = w.carve(sizeof(float) * nlevels);
    const size_t staged = w.used;
    const size_t o_res = w.used;
    const size_t o_mk = w.carve(sizeof(int) * (size_t)P * n), o_nm = w.carve(sizeof(int) * P),
                 o_proj = w.carve(proj ? sizeof(float) * 4 * (size_t)P * m : 1);
    const size_t res_bytes = w.used - o_res;
    if (w.reserve(w.used, std::max(staged, res_bytes))) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation failed");
    map.fill(w);
    fs.fill(w);
    if (has_mappoint && ns) fs.fill_occ(w.h<uint8_t>(o_occ), has_mappoint);
    MapPose *hp = w.h<MapPose>(o_pose);
    for (int p = 0; p < P; ++p) {
        for (int k = 0; k < 9; ++k) hp[p].R[k] = Rcw[9 * p + k];
        for (int k = 0; k < 3; ++k) hp[p].t[k] = tcw[3 * p + k];
    }
    memcpy(w.h<char>(o_sc), scale_factors, sizeof(float) * nlevels);
    hipStream_t st = w.st;
    ORBX_HIP(orbx::stage_in(w.dev, w.pin, staged, st));
    ORBX_HIP(hipMemsetAsync(w.d<char>(o_mk), 0xff, sizeof(int) * (size_t)P * n, st));
    ORBX_HIP(hipMemsetAsync(w.d<char>(o_nm), 0, sizeof(int) * P, st));
    const FrameView fv = fs.view(w);
    hipLaunchKernelGGL(k_map_search_poses, dim3((m + MPP_TILE - 1) / MPP_TILE), dim3(MPP_T), 0, st, map.d_pos(w), map.d_nrm(w), map.d_min(w),
                       map.d_max(w), map.d_desc(w), m, (const MapPose *)w.d<MapPose>(o_pose), P, map_intrinsics(cam, th, nlevels), (const float *)w.d<float>(o_sc), fv.kp,
                       fv.desc, fv.cell_off, fv.perm, has_mappoint && ns ? (const uint8_t *)w.d<uint8_t>(o_occ) : nullptr, fv.gp, n, th_reloc,
                       nnratio, w.d<int>(o_mk), w.d<int>(o_nm), proj ? w.d<float>(o_proj) : nullptr);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(orbx::stage_out(w.pin, w.dev + o_res, res_bytes, st));
    ORBX_HIP(hipStreamSynchronize(st));
    g_last_map_poses_waits.store(1, std::memory_order_relaxed);    // counted where the stream is waited for
    memcpy(matched_mp, w.pin + (o_mk - o_res), sizeof(int) * (size_t)P * n);
    memcpy(nmatches, w.pin + (o_nm - o_res), sizeof(int) * P);
    if (proj) memcpy(proj, w.pin + (o_proj - o_res), sizeof(float) * 4 * (size_t)P * m);
    return ORBX_OK;
}

// What both ..._map_poses entries refuse and preset once their own arguments are checked; *go = there is something to launch.
int map_poses_begin(int n, int m, const double *Rcw, const double *tcw, int P, const orbm_camera *cam, const float *scale_factors,
                    int nlevels, int32_t *matched_mp, int32_t *nmatches, bool octaves_bad, bool *go)
{
    *go = false;
    if (P < 0 || nlevels < 1 || nlevels > 16 || !cam || !scale_factors || (P && (!Rcw || !tcw || !nmatches || (n && !matched_mp))))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (P > MPP_MAXP) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 16 poses in one call");
    if (octaves_bad) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    g_last_map_poses_waits.store(0, std::memory_order_relaxed);
    for (size_t j = 0; j < (size_t)P * n; ++j) matched_mp[j] = -1;
    for (int p = 0; p < P; ++p) nmatches[p] = 0;
    *go = P && n && m;
    return ORBX_OK;
}

} // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ window searches

int orbm_search_window(const orbm_window_query *queries, const uint8_t *qdesc, int nq, const orbx_keypoint *kps,
                       const uint8_t *desc, int n, const uint8_t *skip, const float *uright, float min_x, float min_y,
                       float max_x, float max_y, int init_dist, int32_t *best, int32_t *best_level, int32_t *second,
                       int32_t *second_level, int32_t *idx)
{
    if (nq < 0 || n < 0 || n > 65535 || (nq && (!queries || !qdesc || !best || !best_level || !second || !second_level || !idx)) ||
        (n && (!kps || !desc)) || !(max_x > min_x) || !(max_y > min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(kps, n)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    if (nq == 0) return ORBX_OK;
    SortedFrame sf;
    sort_frame(kps, desc, n, nullptr, uright, min_x, min_y, max_x, max_y, sf);
    FrameSrc fs(sf);
    return search_window_core(fs, queries, qdesc, nq, skip, uright ? 1 : 0, init_dist, nullptr, 0, 0, best, best_level, second, second_level, idx);
}

int orbm_frame_search_window(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, int nq, const uint8_t *skip,
                             int init_dist, int32_t *best, int32_t *best_level, int32_t *second, int32_t *second_level, int32_t *idx)
{
    if (!frame || nq < 0 || (nq && (!queries || !qdesc || !best || !best_level || !second || !second_level || !idx)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (bad_octaves(frame)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    if (nq == 0) return ORBX_OK;
    FrameSrc fs(frame);
    return search_window_core(fs, queries, qdesc, nq, skip, frame->has_uright, init_dist, nullptr, 0, 0, best, best_level, second, second_level, idx);
}

int orbm_search_by_projection_map(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *has_mappoint,
                                  const float *mp_pos, const float *mp_normal, const float *mp_min_dist,
                                  const float *mp_max_dist, const uint8_t *mp_desc, int m, const double *Rcw,
                                  const double *tcw, const orbm_camera *cam, const float *scale_factors, int nlevels,
                                  float th, float nnratio, int th_reloc, int32_t *matched_mp, int *nmatches, float *proj)
{
    if (n < 0 || m < 0 || n > 65535 || nlevels < 1 || nlevels > 64 || !cam || !Rcw || !tcw || !scale_factors || !matched_mp ||
        (n && (!kps || !desc)) || (m && (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc)) ||
        !(cam->grid_max_x > cam->grid_min_x) || !(cam->grid_max_y > cam->grid_min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    for (int j = 0; j < n; ++j) matched_mp[j] = -1;
    if (nmatches) *nmatches = 0;
    if (n == 0 || m == 0) return ORBX_OK;
    SortedFrame sf;
    sort_frame(kps, desc, n, nullptr, nullptr, cam->grid_min_x, cam->grid_min_y, cam->grid_max_x, cam->grid_max_y, sf);
    FrameSrc fs(sf);
    MapSrc map = {mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, nullptr, m};
    return search_map_core(fs, n, has_mappoint, map, Rcw, tcw, cam, scale_factors, nlevels, th, nnratio, th_reloc, matched_mp, nmatches, proj);
}

int orbm_frame_search_by_projection_map(const orbm_frame *frame, const uint8_t *has_mappoint, const float *mp_pos, const float *mp_normal,
                                        const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, int m, const double *Rcw,
                                        const double *tcw, const orbm_camera *cam, const float *scale_factors, int nlevels, float th,
                                        float nnratio, int th_reloc, int32_t *matched_mp, int *nmatches, float *proj)
{
    if (!frame || m < 0 || nlevels < 1 || nlevels > 64 || !cam || !Rcw || !tcw || !scale_factors || !matched_mp ||
        (m && (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    const int n = frame->n;
    for (int j = 0; j < n; ++j) matched_mp[j] = -1;
    if (nmatches) *nmatches = 0;
    if (n == 0 || m == 0) return ORBX_OK;
    FrameSrc fs(frame);
    MapSrc map = {mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, nullptr, m};
    return search_map_core(fs, n, has_mappoint, map, Rcw, tcw, cam, scale_factors, nlevels, th, nnratio, th_reloc, matched_mp, nmatches, proj);
}

// ------------------------------------------------------------------------------------------------ the map as a snapshot

int orbm_map_create(const float *mp_pos, const float *mp_normal, const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc,
                    int m, orbm_map **out)
{
    if (!out || m < 0 || (m && (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc))) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    orbm_map *mp = new orbm_map();
    mp->m = m;
    if (m) {
        // one block: descriptors, positions, normals, the two distances (each part a multiple of 16 bytes behind a 256-byte boundary)
        const size_t b_desc = (size_t)32 * m, b_3 = (sizeof(float) * 3 * m + 255) & ~(size_t)255, b_1 = (sizeof(float) * m + 255) & ~(size_t)255;
        if (hipMalloc((void **)&mp->block, ((b_desc + 255) & ~(size_t)255) + 2 * b_3 + 2 * b_1) != hipSuccess) { delete mp; ORBX_FAIL(ORBX_ERR_HIP, "map allocation failed"); }
        char *p = mp->block;
        mp->desc = reinterpret_cast<uint4 *>(p); p += (b_desc + 255) & ~(size_t)255;
        mp->pos = reinterpret_cast<float *>(p); p += b_3;
        mp->nrm = reinterpret_cast<float *>(p); p += b_3;
        mp->mind = reinterpret_cast<float *>(p); p += b_1;
        mp->maxd = reinterpret_cast<float *>(p);
        const int rc = copy_and_wait({{mp->desc, mp_desc, b_desc}, {mp->pos, mp_pos, sizeof(float) * 3 * m}, {mp->nrm, mp_normal, sizeof(float) * 3 * m},
                                      {mp->mind, mp_min_dist, sizeof(float) * m}, {mp->maxd, mp_max_dist, sizeof(float) * m}}, hipMemcpyHostToDevice);
        if (rc != ORBX_OK) { (void)hipFree(mp->block); delete mp; ORBX_FAIL(ORBX_ERR_HIP, "map upload failed"); }
    }
    *out = mp;
    return ORBX_OK;
}

int orbm_map_destroy(orbm_map *map)
{
    if (!map) return ORBX_OK;
    if (map->block) (void)hipFree(map->block);
    delete map;
    return ORBX_OK;
}

int orbm_map_size(const orbm_map *map, int *m)
{
    if (!map || !m) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    *m = map->m;
    return ORBX_OK;
}

int orbm_search_by_projection_map_poses(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *has_mappoint,
                                        const float *mp_pos, const float *mp_normal, const float *mp_min_dist, const float *mp_max_dist,
                                        const uint8_t *mp_desc, int m, const double *Rcw, const double *tcw, int P, const orbm_camera *cam,
                                        const float *scale_factors, int nlevels, float th, float nnratio, int th_reloc,
                                        int32_t *matched_mp, int32_t *nmatches, float *proj)
{
    if (n < 0 || m < 0 || n > 65535 || (n && (!kps || !desc)) || (m && (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc)) ||
        (cam && (!(cam->grid_max_x > cam->grid_min_x) || !(cam->grid_max_y > cam->grid_min_y))))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    bool go;
    if (const int rc = map_poses_begin(n, m, Rcw, tcw, P, cam, scale_factors, nlevels, matched_mp, nmatches, bad_octaves(kps, n), &go)) return rc;
    if (!go) return ORBX_OK;
    SortedFrame sf;
    sort_frame(kps, desc, n, nullptr, nullptr, cam->grid_min_x, cam->grid_min_y, cam->grid_max_x, cam->grid_max_y, sf);
    FrameSrc fs(sf);
    MapSrc map = {mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, nullptr, m};
    return search_map_poses_core(fs, n, has_mappoint, map, Rcw, tcw, P, cam, scale_factors, nlevels, th, nnratio, th_reloc, matched_mp, nmatches,
                                 proj);
}

int orbm_frame_search_by_projection_map_poses(const orbm_frame *frame, const uint8_t *has_mappoint, const orbm_map *map, const double *Rcw,
                                              const double *tcw, int P, const orbm_camera *cam, const float *scale_factors, int nlevels,
                                              float th, float nnratio, int th_reloc, int32_t *matched_mp, int32_t *nmatches, float *proj)
{
    if (!frame || !map) ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    bool go;
    if (const int rc = map_poses_begin(frame->n, map->m, Rcw, tcw, P, cam, scale_factors, nlevels, matched_mp, nmatches, bad_octaves(frame), &go))
        return rc;
    if (!go) return ORBX_OK;
    FrameSrc fs(frame);
    MapSrc src = {nullptr, nullptr, nullptr, nullptr, nullptr, map, map->m};
    return search_map_poses_core(fs, frame->n, has_mappoint, src, Rcw, tcw, P, cam, scale_factors, nlevels, th, nnratio, th_reloc, matched_mp,
                                 nmatches, proj);
}

int orbm_debug_last_map_poses_waits(void) { return g_last_map_poses_waits.load(std::memory_order_relaxed); }

// Fuse against K target keyframes: one lease, one staged upload (the target records, the list, the mask, the pyramid), one launch
// of k_fuse_keyframes, one result block, one wait.  The kernel writes every pair of the result rows, presets included.
int orbm_fuse_keyframes(const orbm_fuse_target *targets, int K, int sim3, const float *mp_pos, const float *mp_normal,
                        const float *mp_min_distance, const float *mp_max_distance, const uint8_t *mp_desc, int m, const uint8_t *active,
                        float th, float log_scale_factor, const float *scale_factors, const float *inv_level_sigma2, int nlevels,
                        int32_t *best, int32_t *idx, orbm_projected_point *projected)
{
    if (K < 0 || m < 0 || nlevels < 1 || nlevels > 16 || !scale_factors || (!sim3 && !inv_level_sigma2) || (K && !targets) ||
        (m && (!mp_pos || !mp_normal || !mp_min_distance || !mp_max_distance || !mp_desc)) || (K && m && (!best || !idx)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    if (K > 128 || m > 65536 || (size_t)K * (size_t)m > 4194304) ORBX_FAIL(ORBX_ERR_UNSUPPORTED, "more than 128 targets, 65,536 points or 4,194,304 pairs in one call");
    const float *sigma2 = sim3 ? nullptr : inv_level_sigma2;     // the Sim3 form has no reprojection gate
    for (int k = 0; k < K; ++k) {
        const orbm_fuse_target &t = targets[k];
        if (!t.frame) ORBX_FAIL(ORBX_ERR_ARG, "a target without a frame");
        bool finite = true;
        for (int j = 0; j < 9; ++j) finite = finite && isfinite(t.Rcw[j]);
        for (int j = 0; j < 3; ++j) finite = finite && isfinite(t.tcw[j]) && isfinite(t.Ow[j]);
        if (!finite) ORBX_FAIL(ORBX_ERR_ARG, "a target pose that is not finite");
        if (sigma2 && t.frame->n && (t.frame->min_octave < 0 || t.frame->max_octave >= nlevels)) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    }
    ORBX_NEED_DEVICE();
    g_last_fuse_keyframes_waits.store(0, std::memory_order_relaxed);
    if (K == 0 || m == 0) return ORBX_OK;
    const size_t pairs = (size_t)K * m;
    bool any = !active;
    for (size_t j = 0; j < pairs && !any; ++j) any = active[j] != 0;
    if (!any) {         // no active pair: the presets, nothing is launched
        const orbm_projected_point none = {0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
        for (size_t j = 0; j < pairs; ++j) { best[j] = 256; idx[j] = -1; if (projected) projected[j] = none; }
        return ORBX_OK;
    }
    std::vector<FuseTarget> tab((size_t)K);
    for (int k = 0; k < K; ++k) {
        const orbm_fuse_target &t = targets[k];
        const orbm_frame *f = t.frame;
        ProjectCam pc;
        pc.fx = t.cam.fx; pc.fy = t.cam.fy; pc.cx = t.cam.cx; pc.cy = t.cam.cy;
        pc.min_x = t.cam.grid_min_x; pc.max_x = t.cam.grid_max_x; pc.min_y = t.cam.grid_min_y; pc.max_y = t.cam.grid_max_y;     // KeyFrame::IsInImage, as orbm_project_points
        pc.mbf = t.mbf; pc.cos_limit = 0.f; pc.log_scale = log_scale_factor; pc.th = th;
        for (int j = 0; j < 9; ++j) pc.R[j] = t.Rcw[j];
        for (int j = 0; j < 3; ++j) { pc.t[j] = t.tcw[j]; pc.Ow[j] = t.Ow[j]; }
        pc.nlevels = nlevels; pc.mode = sim3 ? ORBM_PROJECT_FUSE_SIM3 : ORBM_PROJECT_FUSE;
        tab[(size_t)k] = {f->kp, f->desc, f->perm, f->cell_off, f->gp, f->has_uright, f->ns, pc};
    }
    StagedCall sc;
    const size_t o_tab = sc.in(tab.data(), sizeof(FuseTarget) * (size_t)K), o_pos = sc.in(mp_pos, sizeof(float) * 3 * m),
                 o_nrm = sc.in(mp_normal, sizeof(float) * 3 * m), o_min = sc.in(mp_min_distance, sizeof(float) * m),
                 o_max = sc.in(mp_max_distance, sizeof(float) * m), o_md = sc.in(mp_desc, (size_t)32 * m), o_act = sc.in(active, active ? pairs : 0),
                 o_sc = sc.in(scale_factors, sizeof(float) * nlevels), o_sg = sc.in(sigma2, sigma2 ? sizeof(float) * nlevels : 0);
    const size_t o_best = sc.out(sizeof(int) * pairs), o_idx = sc.out(sizeof(int) * pairs),
                 o_proj = sc.out(projected ? sizeof(orbm_projected_point) * pairs : 0);
    if (sc.upload()) ORBX_FAIL(ORBX_ERR_HIP, "workspace allocation / upload failed");
    hipLaunchKernelGGL(k_fuse_keyframes, dim3((m + FK_TILE - 1) / FK_TILE, K), dim3(FK_T), 0, sc.stream(), sc.d<const FuseTarget>(o_tab),
                       sc.d<const float>(o_pos), sc.d<const float>(o_nrm), sc.d<const float>(o_min), sc.d<const float>(o_max),
                       sc.d<const uint4>(o_md), m, active ? sc.d<const uint8_t>(o_act) : nullptr, sc.d<const float>(o_sc),
                       sigma2 ? sc.d<const float>(o_sg) : nullptr, sc.d<int>(o_best), sc.d<int>(o_idx),
                       projected ? sc.d<orbm_projected_point>(o_proj) : nullptr);
    ORBX_HIP(hipGetLastError());
    if (sc.download()) ORBX_FAIL(ORBX_ERR_HIP, "download failed");
    g_last_fuse_keyframes_waits.store(sc.waits, std::memory_order_relaxed);    // counted where the stream is waited for
    memcpy(best, sc.r<int>(o_best), sizeof(int) * pairs);
    memcpy(idx, sc.r<int>(o_idx), sizeof(int) * pairs);
    if (projected) memcpy(projected, sc.r<orbm_projected_point>(o_proj), sizeof(orbm_projected_point) * pairs);
    return ORBX_OK;
}

int orbm_debug_last_fuse_keyframes_waits(void) { return g_last_fuse_keyframes_waits.load(std::memory_order_relaxed); }

int orbm_search_fuse(const orbm_window_query *queries, const uint8_t *qdesc, int nq, const orbx_keypoint *kps, const uint8_t *desc,
                     int n, const float *uright, const float *inv_level_sigma2, int nlevels, float min_x, float min_y, float max_x,
                     float max_y, int32_t *best, int32_t *idx)
{
    if (nq < 0 || n < 0 || n > 65535 || (nq && (!queries || !qdesc || !best || !idx)) || (n && (!kps || !desc)) ||
        (inv_level_sigma2 && (nlevels < 1 || nlevels > 64)) || !(max_x > min_x) || !(max_y > min_y))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    for (int j = 0; j < n && inv_level_sigma2; ++j)
        if (kps[j].octave < 0 || kps[j].octave >= nlevels) ORBX_FAIL(ORBX_ERR_ARG, "octave out of range");
    ORBX_NEED_DEVICE();
    if (nq == 0) return ORBX_OK;
    SortedFrame sf;
    sort_frame(kps, desc, n, nullptr, uright, min_x, min_y, max_x, max_y, sf);
    if (!uright) for (SeqKp &k : sf.kp) k.uright = -1.0f;
    FrameSrc fs(sf);
    return search_window_core(fs, queries, qdesc, nq, nullptr, uright ? 1 : 0, 256, inv_level_sigma2, nlevels, 1, best, nullptr, nullptr, nullptr, idx);
}

int orbm_frame_search_fuse(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, int nq,
                           const float *inv_level_sigma2, int nlevels, int32_t *best, int32_t *idx)
{
    if (!frame || nq < 0 || (nq && (!queries || !qdesc || !best || !idx)) || (inv_level_sigma2 && (nlevels < 1 || nlevels > 16)))
        ORBX_FAIL(ORBX_ERR_ARG, "bad arguments");
    ORBX_NEED_DEVICE();
    if (nq == 0) return ORBX_OK;
    FrameSrc fs(frame);
    return search_window_core(fs, queries, qdesc, nq, nullptr, frame->has_uright, 256, inv_level_sigma2, nlevels, 1, best, nullptr, nullptr, nullptr, idx);
}

} // extern "C"
