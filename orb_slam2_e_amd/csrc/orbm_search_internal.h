// orbm_search_internal.h -- what the units of the windowed searches share and nothing else:
//   orbm_frame.hip   makes frames: sorted on the host for one call (sort_frame) or resident in HBM (k_frame_build);
//   orbm_window.hip  searches them with independent queries (k_win_best, k_map_search_poses, k_fuse_keyframes);
//   orbm_search.hip  searches them with the reference's coupled loops (run_sequential), and SearchBySim3 through launch_win_best.
//   orbm_refine_sim3.hip runs SearchBySim3 for a batch of attempts through the two job kernels of those units (PairSearchJob).
// A frame reaches a search as a FrameSrc and its kernels as a FrameView; the projection of a map point (project_point) exists once,
// for k_project_points and k_fuse_keyframes.  What only one unit uses stays in that unit; what the
// other matcher units need as well is in orbm_internal.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "orbm_internal.h"

namespace orbm_detail {

constexpr int SEQ_MAXN = 8192;     // keypoints per frame the resolver's LDS state holds, and a resident frame at most

// Minimum over the wave, in every lane: a butterfly inside each row of 16 lanes on the DPP path (no LDS crossbar round trips),
// then the four row results through scalar registers.  All 64 lanes must be active.
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false));   // row_half_mirror
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false));   // row_mirror
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16),
                   c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// Projection of one map point into a Frame / KeyFrame, in the reference's float / double order, op by op: the one copy of this
// arithmetic, called by k_project_points (orbm_search.hip) and k_fuse_keyframes (orbm_window.hip).
//   mode 0  Frame::isInFrustum (src/Frame.cc:284-340) + MapPoint::PredictScale (src/MapPoint.cc:464-480) and the window
//           of SearchByProjection(Frame&, vector<MapPoint*>&, th) (src/ORBmatcher.cc:62-70, RadiusByViewingCos :332-338)
//   mode 1  the projection block of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, th) (:1053-1094)
//   mode 2  the same block of the Sim3 form (:1212-1250): invz = 1.0 / z in double, no right coordinate
// cv::Mat arithmetic restated (OpenCV 3.4, CV_32F; parity unpinned like the other OpenCV primitives):
//   Rcw * P + tcw  : gemm's 3 x 3 special case -- the row sum a0 b0 + a1 b1 + a2 b2 in float, left to right, then
//                    float(double(sum) + double(t));
//   cv::norm(PO)   : sqrt of the double sum of squares, left to right, cast to float;
//   PO.dot(Pn)     : double sum of double products, left to right.
// std::log / std::ceil on a float argument are the float overloads (using namespace std): logf as glibc >= 2.27 evaluates it,
// restated in orbx_math.h (orbx_logf_glibc_f32: equal to the library at every positive float, tools/trig/logf_count.c; it differs
// from the rounded double logarithm at 416,909 floats -- at none of them by enough to move a level at scale factor 1.2).
struct ProjectCam { float fx, fy, cx, cy, min_x, max_x, min_y, max_y, mbf, cos_limit, log_scale, th; float R[9], t[3], Ow[3]; int nlevels, mode; };

// Point i of the arrays; o and w leave as the rejected record (visible 0, level -1; r < 0: no candidates) unless the point passes
// every test and valid[i] (valid may be NULL).
__device__ __forceinline__ void project_point(int i, const uint8_t *__restrict__ valid, const float *__restrict__ pos, const float *__restrict__ nrm,
                                              const float *__restrict__ mind, const float *__restrict__ maxd, const ProjectCam &cam,
                                              const float *__restrict__ scale, orbm_projected_point &o, WinQuery &w)
{
    o = {0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
    w = {0.f, 0.f, -1.f, 0.f, 0, -1}; // r < 0: no candidates
    const float P0 = pos[3 * i], P1 = pos[3 * i + 1], P2 = pos[3 * i + 2];
    const float *R = cam.R;
    const float PcX = (float)((double)(R[0] * P0 + R[1] * P1 + R[2] * P2) + (double)cam.t[0]);
    const float PcY = (float)((double)(R[3] * P0 + R[4] * P1 + R[5] * P2) + (double)cam.t[1]);
    const float PcZ = (float)((double)(R[6] * P0 + R[7] * P1 + R[8] * P2) + (double)cam.t[2]);
    bool ok = !(PcZ < 0.0f) && (!valid || valid[i]);
    float invz, u, v;
    if (cam.mode == 0) {
        invz = 1.0f / PcZ;                                  // Frame.cc:302-304
        u = cam.fx * PcX * invz + cam.cx;
        v = cam.fy * PcY * invz + cam.cy;
        ok = ok && !(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y);
    } else {
        invz = cam.mode == 1 ? 1 / PcZ : (float)(1.0 / (double)PcZ);   // ORBmatcher.cc:1060 / :1222
        const float x = PcX * invz, y = PcY * invz;
        u = cam.fx * x + cam.cx;
        v = cam.fy * y + cam.cy;
        ok = ok && (u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y); // KeyFrame::IsInImage
    }
    const float ur = u - cam.mbf * invz;
    const float maxDistance = 1.2f * maxd[i], minDistance = 0.8f * mind[i]; // MapPoint.cc:430-440
    const float PO0 = P0 - cam.Ow[0], PO1 = P1 - cam.Ow[1], PO2 = P2 - cam.Ow[2];
    const float dist = (float)sqrt((double)PO0 * (double)PO0 + (double)PO1 * (double)PO1 + (double)PO2 * (double)PO2);
    const double dot = (double)PO0 * (double)nrm[3 * i] + (double)PO1 * (double)nrm[3 * i + 1] + (double)PO2 * (double)nrm[3 * i + 2];
    float viewCos = 0.f;
    if (cam.mode == 0) {
        ok = ok && !((double)dist < 0.9 * (double)minDistance || (double)dist > (double)maxDistance / 0.9);
        viewCos = (float)(dot / (double)dist);
        ok = ok && !(viewCos < cam.cos_limit);
    } else {
        ok = ok && !(dist < minDistance || dist > maxDistance);
        ok = ok && !(dot < 0.5 * (double)dist);
    }
    // PredictScale: ratio = mfMaxDistance / dist; ceil(log(ratio) / mfLogScaleFactor), clamped
    const float ratio = maxd[i] / dist;
    const float lg = orbx_logf_glibc_f32(ratio);        // log(float) = logf under the reference's headers; glibc's logf restated (orbx_math.h)
    int level = orbx_f2i_x86(ceilf(lg / cam.log_scale));   // ratio +inf: INT_MIN -> level 0, as on x86-64
    if (level < 0) level = 0; else if (level >= cam.nlevels) level = cam.nlevels - 1;
    if (ok) {
        o.u = u; o.v = v; o.ur = ur; o.view_cos = viewCos; o.dist = dist; o.level = level; o.visible = 1;
        float r;
        if (cam.mode == 0) {
            r = (double)viewCos > 0.998 ? 3.0f : 4.5f;      // RadiusByViewingCos
            if ((double)cam.th != 1.0) r *= cam.th;
        } else {
            r = cam.th;
        }
        w.u = u; w.v = v; w.r = r * scale[level]; w.xr = ur; w.min_level = level - 1; w.max_level = level;
    }
}

struct SortedFrame {
    std::vector<SeqKp> kp;
    std::vector<int> cell_off; // [COLS*ROWS + 1] runs of the sorted array per grid cell (col * ROWS + row)
    GridParams gp = {0.f, 0.f, 0.f, 0.f};
    std::vector<int> perm;
    std::vector<float> angle;
    std::vector<uint8_t> desc;
};

// Keypoints in the grid (and not excluded by `skip`), ordered by (cell, index).  (orbm_frame.hip)
void sort_frame(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *skip, const float *uright, float min_x,
                float min_y, float max_x, float max_y, SortedFrame &sf);

// What the search kernels read of a frame, wherever it lives.
struct FrameView {
    const SeqKp *kp; const uint4 *desc; const float *angle; const int *perm; const int *cell_off;
    GridParams gp;
};

// The frame of a call: sorted on the host and staged with the call's inputs (the host-array entry points), or resident.
struct FrameSrc {
    const SortedFrame *host = nullptr;
    const orbm_frame *res = nullptr;
    size_t o_k = 0, o_b = 0, o_kang = 0, o_perm = 0, o_cell = 0;
    bool all_positions = false;     // resident frame addressed by explicit candidate lists: the positions behind the grid's count too
    explicit FrameSrc(const SortedFrame &sf) : host(&sf) {}
    explicit FrameSrc(const orbm_frame *f, bool all = false) : res(f), all_positions(all) {}
    int ns() const { return host ? (int)host->perm.size() : (all_positions ? res->n : res->ns); }
    const int *perm() const { return host ? host->perm.data() : res->perm_host.data(); }
    void carve(Workspace &w)
    {
        if (!host) return;
        const size_t m = ns() ? (size_t)ns() : 1;
        o_k = w.carve(sizeof(SeqKp) * m); o_b = w.carve(32 * m); o_kang = w.carve(sizeof(float) * m); o_perm = w.carve(sizeof(int) * m);
        o_cell = w.carve(sizeof(int) * (FRAME_GRID_COLS * FRAME_GRID_ROWS + 1));
    }
    void fill(Workspace &w) const
    {
        if (!host) return;
        const size_t m = (size_t)ns();
        if (!host->kp.empty()) memcpy(w.h<char>(o_k), host->kp.data(), sizeof(SeqKp) * m);
        if (!host->cell_off.empty()) memcpy(w.h<char>(o_cell), host->cell_off.data(), sizeof(int) * host->cell_off.size());
        memcpy(w.h<char>(o_b), host->desc.data(), 32 * m);
        memcpy(w.h<char>(o_kang), host->angle.data(), sizeof(float) * m);
        memcpy(w.h<char>(o_perm), host->perm.data(), sizeof(int) * m);
    }
    FrameView view(const Workspace &w) const
    {
        if (host) return {w.d<SeqKp>(o_k), w.d<uint4>(o_b), w.d<float>(o_kang), w.d<int>(o_perm), w.d<int>(o_cell), host->gp};
        return {res->kp, res->desc, res->angle, res->perm, res->cell_off, res->gp};
    }
    // occupancy by keypoint index -> by sorted position
    void fill_occ(uint8_t *dst, const uint8_t *occupied) const
    {
        const int m = ns();
        const int *pm = perm();
        for (int s = 0; s < m; ++s) dst[s] = occupied[pm[s]];
    }
};

// A candidate entry holds its keypoint's octave in four bits (k_win_wave, entry_level; k_win_best packs it the same way): a frame
// with an octave outside 0..15 cannot be searched.
inline bool bad_octaves(const orbx_keypoint *kps, int n)
{
    for (int j = 0; j < n; ++j)
        if (kps[j].octave < 0 || kps[j].octave > 15) return true;
    return false;
}
inline bool bad_octaves(const orbm_frame *f) { return f->n && (f->min_octave < 0 || f->max_octave > 15); }

// One window search without coupling (k_win_best, orbm_window.hip) for device-resident queries: returns into ob[5][nq] (best, best
// level, second, second level, idx).
void launch_win_best(hipStream_t st, const WinQuery *dq, const uint4 *da, int nq, const FrameView &fv, const uint8_t *docc, int has_uright,
                     int init_dist, const float *inv_sigma2, int fuse_gate, int *ob);

// ---- The projection prefixes of the whole-function searches (k_project_form, orbm_search.hip): the form and what it reads of the
// view, the searched frame and the poses.
enum { FORM_LAST = 0, FORM_KF = 1, FORM_SIM3 = 2, FORM_PAIR = 3 };
struct FormCam {
    float fx, fy, cx, cy, min_x, max_x, min_y, max_y, mbf, log_scale, th;
    float R[9], t[3], Ow[3];      // Rcw, tcw, Ow  (FORM_PAIR: Ra, ta = first transform)
    float R2[9], t2[3];           // FORM_PAIR: the second transform (sR21, t21 / sR12, t12)
    int nlevels, form, forward, backward;
};

inline void form_cam_common(FormCam &c, const orbm_view *v, const orbm_frame *f, int form, float th)
{
    memset(&c, 0, sizeof(c));
    c.fx = v->fx; c.fy = v->fy; c.cx = v->cx; c.cy = v->cy;
    c.min_x = f->min_x; c.max_x = f->max_x; c.min_y = f->min_y; c.max_y = f->max_y;
    c.mbf = v->mbf; c.log_scale = v->log_scale_factor; c.th = th; c.nlevels = v->nlevels; c.form = form;
}

inline bool bad_view(const orbm_view *v) { return !v || !v->scale_factors || v->nlevels < 1 || v->nlevels > 16; }
inline bool bad_points(const orbm_points *p, bool need_range, bool need_normal, bool need_octave, int nlevels)
{
    if (!p || p->n < 0 || p->n > 65536) return true;
    if (p->n == 0) return false;
    if (!p->valid || !p->pos || !p->desc) return true;
    if (need_range && (!p->min_distance || !p->max_distance)) return true;
    if (need_normal && !p->normal) return true;
    if (need_octave) {
        if (!p->octave) return true;
        for (int i = 0; i < p->n; ++i)
            if (p->valid[i] && (p->octave[i] < 0 || p->octave[i] >= nlevels)) return true;
    }
    return false;
}

// The two cameras of SearchBySim3: c12 takes KF1's points into KF2 (src/ORBmatcher.cc:1348-1428), c21 KF2's into KF1 (:1430-1507).
inline void form_pair_cams(FormCam &c12, FormCam &c21, const orbm_view *view, const orbm_frame *kf1, const orbm_frame *kf2, const float *T1w,
                           const float *T2w, float s12, const float *R12, const float *t12, float th)
{
    form_cam_common(c12, view, kf2, FORM_PAIR, th);
    form_cam_common(c21, view, kf1, FORM_PAIR, th);
    pose_parts(T1w, c12.R, c12.t);
    pose_parts(T2w, c21.R, c21.t);
    // :1320-1323: sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12
    float R12t[9];
    scale_mat(R12, 9, (double)s12, c21.R2);
    memcpy(c21.t2, t12, sizeof(float) * 3);
    transpose3(R12, R12t);
    scale_mat(R12t, 9, 1.0 / (double)s12, c12.R2);
    gemm3(c12.R2, t12, -1.0, nullptr, 0.0, c12.t2);
}

// SearchBySim3's acceptance of a direction's best candidate (:1426-1429, :1505-1507) and the agreement of the two (:1509-1524)
__device__ __forceinline__ int sim3_accepted(int best, int idx, int th_high) { return idx >= 0 && best <= th_high ? idx : -1; }
__device__ __forceinline__ bool sim3_agreed(int i1, int a, const int *__restrict__ best2, const int *__restrict__ idx2, int n2, int th_high)
{
    return a >= 0 && a < n2 && sim3_accepted(best2[a], idx2[a], th_high) == i1;
}

// One direction of one SearchBySim3 of a batch (orbm_refine_sim3.hip), as a record in the call's staged block: o_* are byte offsets
// in the workspace.  k_project_pair_jobs (orbm_search.hip) turns the nq list entries into queries, k_win_best_jobs (orbm_window.hip)
// searches `frame` with them: best [nq] (INT_MAX when absent) and idx [nq] (keypoint index, -1).
struct PairSearchJob {
    FormCam cam;
    FrameView frame;
    unsigned o_valid, o_pos, o_min, o_max, o_desc;  // the list: valid as the search sees it, pos, the distance bounds, descriptors
    unsigned o_q, o_best, o_idx;                    // scratch: queries, results
    int nq;
};
void launch_project_pair_jobs(hipStream_t st, const PairSearchJob *djobs, int njobs, int max_nq, char *ws, const float *dscale);
void launch_win_best_jobs(hipStream_t st, const PairSearchJob *djobs, int njobs, int max_nq, char *ws);

// Copies outside a call's staged traffic (a resident frame's arrays for an accessor, a snapshot's upload), all in one direction: on
// the own stream of a leased workspace, like every other call, waited for once.
struct CopyJob { void *dst; const void *src; size_t bytes; };
inline int copy_and_wait(std::initializer_list<CopyJob> jobs, hipMemcpyKind kind)
{
    WorkspaceLease lease;
    const hipStream_t st = lease.w->own_stream();
    if (!st) ORBX_FAIL(ORBX_ERR_HIP, "hipStreamCreate failed");
    for (const CopyJob &j : jobs) ORBX_HIP(hipMemcpyAsync(j.dst, j.src, j.bytes, kind, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return ORBX_OK;
}

} // namespace orbm_detail
