/*
 * orbslam_hip.h -- C ABI of the MI355X-native front-end hot path of ORB_SLAM2_E.
 *
 * One shared library (liborbslam_hip.so), plain pointers and sizes, int status
 * codes, never throws.  Each entry point names the reference interface it
 * replaces (paths relative to the ORB_SLAM2_E tree).  INTEGRATION.md shows the
 * reference-side C++ binding (ORBextractor / ORBmatcher / FEA2 shells).
 *
 * Conventions
 *   - `*_dev` pointers are device (HBM) addresses, everything else is host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the handle's own stream).
 *   - Status: 0 = ORBX_OK, negative = error (see enum).  No CPU fallback exists:
 *     without a usable HIP device every compute call returns ORBX_ERR_NO_DEVICE.
 */
#ifndef ORBSLAM_HIP_H
#define ORBSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ORBX_OK = 0,
    ORBX_ERR_ARG = -1,        /* null pointer, bad size, image too small for the 30-px cell grid */
    ORBX_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime failure at init */
    ORBX_ERR_HIP = -3,        /* a HIP call failed; orbx_last_error() has the text */
    ORBX_ERR_CAPACITY = -4,   /* caller buffer or configured capacity too small */
    ORBX_ERR_UNSUPPORTED = -5 /* parameter outside the supported range */
};

const char *orbx_last_error(void);
/* ABI version of this header (major*100+minor).  136 (additions only): the pose-only optimisation (orbm_pose_*).  Added since
 * without a new number (additions only): orbm_create_new_map_points, orbm_debug_last_create_points_waits; orbm_sim3_hypotheses,
 * orbm_debug_last_sim3_waits; orbm_optimize_sim3, orbm_debug_last_sim3_opt_waits; orbm_map_create / _destroy / _size,
 * orbm_search_by_projection_map_poses, orbm_frame_search_by_projection_map_poses, orbm_debug_last_map_poses_waits;
 * orbm_init_find_models, orbm_init_check_rt, orbm_init_reconstruct_f, orbm_debug_last_init_waits, orbm_debug_init_svd;
 * orbm_fuse_keyframes, orbm_debug_last_fuse_keyframes_waits; orbm_pnp_hypotheses, orbm_debug_last_pnp_waits, orbm_debug_pnp_pose;
 * orbm_debug_fill_workspaces, orbm_debug_last_search_waits; orbm_bundle_adjustment, orbm_ba_plan, orbm_debug_last_ba_waits;
 * orbm_global_bundle_adjustment, orbm_global_ba_plan, orbm_llt_tile, orbm_llt_solve_dev, orbm_debug_last_llt_launches;
 * orbm_essential_graph, orbm_eg_plan, orbm_debug_last_eg_waits; orbm_refine_sim3_candidates, orbm_debug_last_refine_sim3_waits;
 * orbm_llt_env_plan, orbm_llt_env_solve_dev, orbm_essential_graph_env, orbm_eg_env_plan; orbm_global_bundle_adjustment_env,
 * orbm_global_ba_env_plan. */
int orbx_abi_version(void);

/* ------------------------------------------------------------------ extractor
 * Replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:46-112,
 * src/ORBextractor.cc:410-470 ctor, :1051-1113 operator()).                   */

/* Same 28-byte layout as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id). */
typedef struct orbx_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

typedef struct orbx_params {
    int32_t nfeatures;     /* ORBextractor ctor arg 1 */
    float scale_factor;    /* arg 2 */
    int32_t nlevels;       /* arg 3 (1..16) */
    int32_t ini_th_fast;   /* arg 4 */
    int32_t min_th_fast;   /* arg 5 */
    int32_t blur_variant;  /* 0: 7-tap 8.8 kernel {18,34,48,56,48,34,18} (sum 256, canonical);
                              1: {18,34,49,55,49,34,18} (taps rounded individually) */
    int32_t trig_variant;  /* cos / sin of the keypoint angle in computeOrbDescriptor (ORBextractor.cc:111-113: a float argument under
                              `using namespace std`, i.e. cosf / sinf):
                              0: cosf / sinf as glibc >= 2.28 computes them (any current Linux; bit-exact restatement, checked over
                                 every float in [0, 2 pi] by tools/trig/trig_variant_count.c);
                              1: the correctly rounded float of the double-precision cos / sin (differs from 0 by one ulp at 0.36 % /
                                 0.83 % of the angles: DESIGN 4.2) */
} orbx_params;

typedef struct orbx_extractor orbx_extractor;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) */
int orbx_create(const orbx_params *params, orbx_extractor **out);
int orbx_destroy(orbx_extractor *ex);

/* Getters: ORBextractor.h:61-84 (GetLevels, GetScaleFactors, GetInverseScaleFactors,
 * GetScaleSigmaSquares, GetInverseScaleSigmaSquares) + mnFeaturesPerLevel (:97). */
int orbx_get_levels(const orbx_extractor *ex);
int orbx_get_scale_factors(const orbx_extractor *ex, float *out_nlevels);
int orbx_get_inv_scale_factors(const orbx_extractor *ex, float *out_nlevels);
int orbx_get_level_sigma2(const orbx_extractor *ex, float *out_nlevels);
int orbx_get_inv_level_sigma2(const orbx_extractor *ex, float *out_nlevels);
int orbx_get_features_per_level(const orbx_extractor *ex, int32_t *out_nlevels);
/* Upper bound on keypoints per frame: nfeatures + 3*nlevels. */
int orbx_keypoint_capacity(const orbx_extractor *ex);

/* Size the device workspace for `batch` frames of width x height (idempotent;
 * called implicitly by the extract calls). */
int orbx_reserve(orbx_extractor *ex, int width, int height, int batch);

/* What orbx_reserve decides about a frame size, computed on the host alone (no device needed): level sizes
 * (ComputePyramid, ORBextractor.cc:1119-1121), quotas, DistributeOctTree's initial nodes round(W / H) per level (:543), the
 * keypoint slots of a level = max(quota + 3, 4 nIni) + 1, the frame's keypoint capacity, the FAST cell count per level
 * (:781-806) and the workspace / LDS budgets.  Same error codes as orbx_reserve for sizes it refuses. */
typedef struct {
    int32_t nlevels, keypoint_capacity, octree_nodes, cells_per_frame, sel_per_frame, fast_tile_stride, fast_lds, octree_lds, octree_kshift, reserved;
    int64_t frame_bytes, cands_per_frame;
    int32_t level_w[16], level_h[16], level_quota[16], level_nini[16], level_slots[16], level_cells[16];
} orbx_plan_info;
int orbx_plan(const orbx_params *params, int width, int height, orbx_plan_info *info);

/* Development aid, host alone like orbx_plan: what k_fast_cells' tile load reads of a frame's pyramid block, FAST cell by cell in
 * grid order.  Eight int32 per cell: level, byte offset of the cell's first piece in the frame's block, row pitch, rows read,
 * 16-byte pieces read per row (rows and pieces 0: a cell without a zone loads nothing), cell width, cell origin x0, y0 in level
 * coordinates.  *n = cells of a frame; ORBX_ERR_CAPACITY if `cap` cells are too few. */
int orbx_debug_fast_pieces(const orbx_params *params, int width, int height, int32_t *out, int cap, int *n);

/* ORBextractor::operator()(image, mask, keypoints, descriptors) for ONE host image
 * (CV_8UC1, `stride` bytes per row).  Writes up to `cap` keypoints / 32-byte
 * descriptor rows; *n = count.  An empty image (NULL / 0 size) returns ORBX_OK
 * with outputs untouched and *n = 0 (ORBextractor.cc:1054-1055). */
int orbx_extract(orbx_extractor *ex, const uint8_t *image, int width, int height, int stride,
                 orbx_keypoint *kps, uint8_t *desc, int cap, int *n);

/* The two images of a stereo frame (Frame.cc:78-81: ExtractORB on two threads, then join) in one call from one host thread:
 * both kernel chains are enqueued on their handles' streams before the host waits for either, so they overlap on the
 * device as the reference's threads overlap on the CPU.  Results as from two orbx_extract calls (left != right; same
 * error behaviour).  Frame::ComputeStereoMatches = orbx_stereo_match on the two handles afterwards. */
int orbx_extract_pair(orbx_extractor *left, const uint8_t *image_left, orbx_extractor *right, const uint8_t *image_right, int width,
                      int height, int stride, orbx_keypoint *kps_left, uint8_t *desc_left, int cap_left, int *n_left,
                      orbx_keypoint *kps_right, uint8_t *desc_right, int cap_right, int *n_right);

/* Batch form: `batch` frames, frame f at images + f*frame_stride.  images_dev may
 * be a device pointer (is_device=1: inputs already resident in HBM) or host.
 * Results stay on the device until orbx_download / orbx_result_dev. Asynchronous
 * on `stream`. */
int orbx_extract_batch(orbx_extractor *ex, const uint8_t *images, int is_device,
                       int width, int height, int stride, size_t frame_stride, int batch, void *stream);
/* Copy frame f's result of the last batch to host (synchronises the stream). */
int orbx_download(orbx_extractor *ex, int frame, orbx_keypoint *kps, uint8_t *desc, int cap, int *n);
/* Whole last batch to host in three copies: kps[batch][capacity],
 * desc[batch][capacity][32], counts[batch]; any pointer may be NULL. */
int orbx_download_batch(orbx_extractor *ex, orbx_keypoint *kps, uint8_t *desc, int32_t *counts);
/* Device-side result arrays of the last batch: kps[batch][capacity],
 * desc[batch][capacity][32], counts[batch] (int32). */
int orbx_result_dev(orbx_extractor *ex, const orbx_keypoint **kps_dev, const uint8_t **desc_dev,
                    const int32_t **counts_dev, int *capacity);

/* Asynchronous export of the last batch's result arrays into caller-owned buffers
 * (same shapes as orbx_result_dev) -- device memory, or pinned host memory for a
 * download that overlaps the next batch; any pointer may be NULL.  Used to stage the
 * fixed-size records of the multi-GPU gather. */
int orbx_copy_results_dev(orbx_extractor *ex, orbx_keypoint *kps_dst_dev, uint8_t *desc_dst_dev,
                          int32_t *counts_dst_dev, void *stream);

/* mvImagePyramid[level] of frame f of the last call (ORBextractor.h:86; read by
 * Frame::ComputeStereoMatches, src/Frame.cc:534,624,636,641): copies the level
 * image (without border) into out[height][out_stride]. */
int orbx_level_size(const orbx_extractor *ex, int level, int *width, int *height);
int orbx_pyramid_level(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride);
/* Same with the 19-px REFLECT_101 border: out[(h+38)][out_stride], width w+38. */
int orbx_pyramid_level_padded(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride);

/* Frame::ComputeStereoMatches (src/Frame.cc:527-701) for every frame of the last
 * batch extracted on `left` and `right` (two distinct handles with the same
 * parameters, Frame.cc:78-81): row-band Hamming match (+-1 octave, disparity in
 * [0, mbf/mb]), 11x11 L1 sub-pixel refinement on the keypoint's pyramid level,
 * median cut.  Results stay on the device in the left handle; download returns
 * mvuRight[n] / mvDepth[n] (-1 where unmatched) for one frame.  An extraction that makes
 * orbx_reserve lay the left handle out anew (another frame size, or a larger batch)
 * invalidates its stereo results: orbx_stereo_download, orbx_stereo_download_batch and
 * orbm_frame_from_extractor(..., uright_from_stereo = 1) return ORBX_ERR_ARG ("no stereo
 * results") until the next orbx_stereo_match.  A new extraction at the same size keeps
 * them (they then describe the earlier images). */
int orbx_stereo_match(orbx_extractor *left, orbx_extractor *right, float mb, float mbf, void *stream);
int orbx_stereo_download(orbx_extractor *left, int frame, float *uRight, float *depth, int cap, int *n);
/* All frames of the last orbx_stereo_match at once: uRight / depth [batch][capacity] (rows past a frame's count are
 * unspecified), counts[batch] = the left keypoint counts; any of the three may be NULL. */
int orbx_stereo_download_batch(orbx_extractor *left, float *uRight, float *depth, int32_t *counts);

/* Staged outputs for parity tests (no reference counterpart; they expose the
 * intermediate values the reference keeps in locals):
 *   blurred level image (GaussianBlur output, ORBextractor.cc:1093-1094),
 *   FAST candidates per level = vToDistributeKeys (:826-834) as (x,y,response) triples,
 *   per-level keypoints after DistributeOctTree + orientation (:842-860). */
int orbx_debug_blurred_level(orbx_extractor *ex, int frame, int level, uint8_t *out, int out_stride);
int orbx_debug_level_candidates(orbx_extractor *ex, int frame, int level, float *xyr, int cap, int *n);
int orbx_debug_level_keypoints(orbx_extractor *ex, int frame, int level, orbx_keypoint *kps, int cap, int *n);

/* Per-kernel timing with HIP events on the launch stream (no reference
 * counterpart; feeds bench.py's roofline object).  `on`: 0 = off, < 0 = every
 * kernel kind, > 0 = bit mask of kinds (bit i = i-th name returned by read): each
 * recorded event widens the dispatch gap by a few microseconds, so a timed run
 * enables only the kernel it reports.  Read returns, per kernel kind, its name,
 * accumulated milliseconds and launch count since enable. */
int orbx_profile_enable(orbx_extractor *ex, int on);
int orbx_profile_read(orbx_extractor *ex, int max_kinds, const char **names, double *total_ms,
                      int64_t *launches, int *nkinds);

/* -------------------------------------------------------------------- matcher
 * Data plane of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:37-111).            */

/* Counts that become the y dimension of a launch grid.  The device's limit is hipDeviceProp_t::maxGridSize[1]; the library
 * relies on no more than 65,535 there, the smallest value a HIP platform reports: orbm_match_batch_dev (npairs) and orbm_bow_transform_batch_dev (nsets) refuse a
 * larger count with ORBX_ERR_UNSUPPORTED before anything is queued; orbm_hamming_matrix takes any nA (its kernel strides
 * over the rows). */
#define ORBM_MAX_GRID_Y 65535

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1848-1864) for all pairs:
 * out[nA][nB] uint16.  Host pointers; runs on the device.  Any nA, nB >= 0 whose product fits the device. */
int orbm_hamming_matrix(const uint8_t *A, int nA, const uint8_t *B, int nB, uint16_t *out);

/* Best / second-best / arg-best per query row over all of B, first index wins
 * ties -- the selection loop shared by every ORBmatcher::Search* (e.g.
 * ORBmatcher.cc:645-672).  best/second = INT32_MAX and idx = -1 when nB == 0. */
int orbm_match_bruteforce(const uint8_t *A, int nA, const uint8_t *B, int nB,
                          int32_t *best, int32_t *second, int32_t *idx);
/* Same over gated candidate lists (CSR: cand_off[nA+1], cand_idx[] in
 * GetFeaturesInArea / BoW-member order). */
int orbm_match_candidates(const uint8_t *A, int nA, const uint8_t *B, int nB,
                          const int32_t *cand_off, const int32_t *cand_idx,
                          int32_t *best, int32_t *second, int32_t *idx);
/* Frame::GetFeaturesInArea(u, v, r, minLevel, maxLevel) (src/Frame.cc:342-395, on
 * the 64x48 grid of Frame::AssignFeaturesToGrid :245-260) fused with the best /
 * second-best-with-levels loop that the SearchByProjection family runs over its
 * result (ORBmatcher.cc:69-118; same shape at :166-205, :1600-1640, :1730-1770).
 * kps = mvKeysUn, (min_x..max_y) = mnMinX..mnMaxY; skip[j] != 0 excludes keypoint j
 * (already holds an observed MapPoint, :87-89); uright (may be NULL) enables the
 * stereo check |xr - uRight[j]| <= r of :91-96.  init_dist: 256 or INT32_MAX.
 * Outputs per query: best / second distance, their octaves, arg-best (-1 if none).
 * Queries are independent here; the loops that assign matches as they go (e.g. :126
 * F.mvpMapPoints[bestIdx]=pMP) are orbm_search_projection and the whole-function entries below. */
typedef struct orbm_window_query {
    float u, v, r, xr;
    int32_t min_level, max_level;
} orbm_window_query;
int orbm_search_window(const orbm_window_query *queries, const uint8_t *qdesc, int nq, const orbx_keypoint *kps,
                       const uint8_t *desc, int n, const uint8_t *skip, const float *uright, float min_x, float min_y,
                       float max_x, float max_y, int init_dist, int32_t *best, int32_t *best_level, int32_t *second,
                       int32_t *second_level, int32_t *idx);

/* Candidate loop of ORBmatcher::Fuse (src/ORBmatcher.cc:1092-1146; Sim3 form :1245-1276): per map point that passed
 * the caller's projection / distance / viewing-angle tests, the window (u, v, r), levels [min_level, max_level] =
 * [l-1, l], xr = ur; a keypoint is scored only if its reprojection error passes e2 * inv_level_sigma2[level] <= 7.8
 * (stereo keypoint, uright[j] >= 0: ex, ey, er) or <= 5.99 (mono: ex, ey) -- inv_level_sigma2 = NULL switches the
 * gate off (the Sim3 form has none).  best[i] = smallest distance (256 if none), idx[i] = its keypoint (-1).  The map
 * update that follows in the reference (:1149-1170: Replace / AddObservation, nFused) reads only these two values
 * and stays on the host, in the reference's order. */
int orbm_search_fuse(const orbm_window_query *queries, const uint8_t *qdesc, int nq, const orbx_keypoint *kps, const uint8_t *desc,
                     int n, const float *uright, const float *inv_level_sigma2, int nlevels, float min_x, float min_y, float max_x,
                     float max_y, int32_t *best, int32_t *idx);

/* The SearchByProjection family as whole loops: the selection of orbm_search_window plus
 * what the reference does between queries and after them,
 *   SearchByProjection(Frame&, vector<MapPoint*>&, th)          src/ORBmatcher.cc:46-132
 *       th_accept = TH_HIGH, ratio_same_level = 1 (:121), check_orientation = 0
 *   SearchByProjection(CurrentFrame, LastFrame, th, bMono)      :1529-1671   TH_HIGH, 0, mbCheckOrientation
 *   SearchByProjection(CurrentFrame, KeyFrame*, found, th, d)   :1673-1800   ORBdist, 0, mbCheckOrientation
 *   SearchByProjection(KeyFrame*, Scw, points, matched, th)     :491-604     TH_LOW,  0, 0
 * Query i = one map point that passed the caller's projection / frustum tests, in the
 * caller's loop order: its window and level range (as orbm_search_window), xr = u - bf/z,
 * its descriptor (MapPoint::GetDescriptor), qangle[i] = angle of its source keypoint (only
 * read when check_orientation), qtakes[i] != 0 when the pointer it leaves in
 * mvpMapPoints[best] makes later queries skip that keypoint (Observations() > 0 in the
 * first two forms; NULL = always, the last two).  occupied[j] != 0: keypoint j is skipped
 * from the start.  Each query sees the assignments of the queries before it, exactly as
 * the sequential loop (:87-89, :1603-1605, :1741-1742, :574-575).  Then the 30-bin rotation
 * histogram, ComputeThreeMaxima (:1802-1843) and the rejection of the other bins.
 * match_kp[j] = query whose point ends in slot j, -1 = slot untouched, -2 = slot set to
 * NULL by the rotation check; match_q[i] = keypoint chosen by query i when it was accepted
 * (before the rotation check) or -1; *nmatches as the reference counts it.
 * Limits: at most 8192 keypoints inside the grid, 65536 queries.  A keypoint octave outside 0..15 in the searched frame is
 * ORBX_ERR_ARG ("octave out of range") here, in orbm_search_window, orbm_search_for_initialization, their resident-frame
 * forms and the whole-function entries: a candidate entry holds the octave in four bits. */
int orbm_search_projection(const orbm_window_query *queries, const uint8_t *qdesc, const float *qangle, const uint8_t *qtakes,
                           int nq, const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *occupied,
                           const float *uright, float min_x, float min_y, float max_x, float max_y, int th_accept, float nnratio,
                           int ratio_same_level, int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cc:606-721), whole: level-0 keypoints of F1, window around
 * vbPrevMatched[i1] on level 0 of F2 (grid bounds = F2's mnMinX..mnMaxY), candidates whose
 * vMatchedDistance is not above the new distance are skipped (:645-646), best <= TH_LOW and
 * best < second * nnratio, a better match steals the keypoint (:678-682), rotation
 * histogram over every accepted match (stolen ones included, as the reference pushes
 * them), ComputeThreeMaxima, rejection, vbPrevMatched update (:715-718).  kps1 / kps2 =
 * mvKeysUn.  matches12[n1] = vnMatches12; prev_matched[n1][2] in/out. */
int orbm_search_for_initialization(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbx_keypoint *kps2,
                                   const uint8_t *desc2, int n2, float *prev_matched, float min_x, float min_y, float max_x,
                                   float max_y, int window_size, float nnratio, int check_orientation, int32_t *matches12,
                                   int *nmatches);

/* ORBmatcher::SearchByBoW, both forms, as a whole loop:
 *   SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches)   src/ORBmatcher.cc:360-489  valid2 = NULL, th = TH_LOW, strict_th = 0 (:429)
 *   SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)      :723-856                   valid2 given, th = TH_LOW, strict_th = 1 (:799)
 * A DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>) is passed flat, in map order:
 * nodes[nn] ascending, members of node k = items[off[k] .. off[k+1]) in insertion order.
 * valid1[i] != 0: feature i of the first keyframe owns a good MapPoint (:395-399, :763-767);
 * valid2 likewise for the second keyframe (:782-786).  The lower_bound co-iteration of
 * :384-456 runs on the host; then, in the reference's visiting order, every feature of the
 * first set selects best / second (from 256) over the members of its node in the second
 * set that no earlier feature has matched (:415-416, :784), accepts on best <= th (< th if
 * strict_th) and (float)best < nnratio * (float)second; rotation histogram +
 * ComputeThreeMaxima + rejection.  match12[n1] = feature of the second set or -1;
 * match21[n2] (may be NULL) the inverse; *nmatches as the reference returns it.
 * At most 8192 features in the second set. */
int orbm_search_by_bow(const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1, const uint8_t *valid1,
                       const uint8_t *desc1, const float *angle1, int n1, const int32_t *nodes2, const int32_t *off2,
                       const int32_t *items2, int nn2, const uint8_t *valid2, const uint8_t *desc2, const float *angle2, int n2,
                       int th, int strict_th, float nnratio, int check_orientation, int32_t *match12, int32_t *match21,
                       int *nmatches);

/* The fork's whole-map relocalisation search, ORBmatcher::SearchByProjection(Frame&,
 * Map*, double Rcw[3][3], double tcw[3], ...) (src/ORBmatcher.cc:134-222): for
 * EVERY map point isInFrustum (:262-330, with ComputeDistance :224-260; mixed
 * float / double arithmetic reproduced operation by operation), level prediction
 * by lower_bound on the scale factors, window r = RadiusByViewingCos * th *
 * scale[level], GetFeaturesInArea(u, v, r, level-1, level), best / second with
 * levels over keypoints that hold no MapPoint, bestDist <= th_reloc and the
 * same-level ratio test.  matched_mp[j] = index of the (last) map point assigned
 * to keypoint j or -1 (vMatchedMPs); *nmatches as the reference counts them.
 * cam: intrinsics, GetImageBounds() ints, grid bounds mnMinX..mnMaxY.  proj
 * (optional, [m][4]): u, v, viewCos, level per map point (level -1 = culled). */
typedef struct orbm_camera {
    float fx, fy, cx, cy;
    int32_t min_x, max_x, min_y, max_y;
    float grid_min_x, grid_min_y, grid_max_x, grid_max_y;
} orbm_camera;
int orbm_search_by_projection_map(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *has_mappoint,
                                  const float *mp_pos, const float *mp_normal, const float *mp_min_dist,
                                  const float *mp_max_dist, const uint8_t *mp_desc, int m, const double *Rcw,
                                  const double *tcw, const orbm_camera *cam, const float *scale_factors, int nlevels,
                                  float th, float nnratio, int th_reloc, int32_t *matched_mp, int *nmatches, float *proj);

/* Batch projection of map points (M15): replaces the per-point host loop in front of every SearchByProjection /
 * Fuse form.  mode ORBM_PROJECT_FRUSTUM = Frame::isInFrustum (src/Frame.cc:284-340: positive depth, image bounds
 * mnMinX..mnMaxY inclusive, distance in [0.9 min, max / 0.9], viewing cosine >= viewing_cos_limit) with
 * MapPoint::PredictScale (src/MapPoint.cc:464-480) -> mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos, and the
 * window of SearchByProjection(Frame&, vector<MapPoint*>&, th) (src/ORBmatcher.cc:62-70: RadiusByViewingCos, * th
 * unless th == 1, * mvScaleFactors[level], levels [l-1, l], xr = mTrackProjXR);
 * ORBM_PROJECT_FUSE = the projection block of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:1053-1094: KeyFrame::IsInImage, distance in [min, max], PO.Pn >= 0.5 dist, radius th *
 * mvScaleFactors[level]); ORBM_PROJECT_FUSE_SIM3 = the Sim3 form (:1212-1250; the caller passes Rcw = sRcw / s,
 * tcw = t / s, Ow = -Rcw' tcw as :1188-1192 computes them).
 * mp_min_distance / mp_max_distance are MapPoint::mfMinDistance / mfMaxDistance (the 0.8 / 1.2 factors of
 * Get{Min,Max}DistanceInvariance are applied here); Rcw row-major 3x3, tcw, Ow = camera centre, all float as the
 * cv::Mat members are; cam->grid_* = mnMinX .. mnMaxY; log_scale_factor = mfLogScaleFactor.
 * out[i].visible = 0 for a point the reference rejects (then level = -1 and queries[i].r < 0 = "no candidates", so
 * the arrays feed orbm_search_projection / orbm_search_fuse as they are).  queries may be NULL. */
enum { ORBM_PROJECT_FRUSTUM = 0, ORBM_PROJECT_FUSE = 1, ORBM_PROJECT_FUSE_SIM3 = 2 };
typedef struct orbm_projected_point {
    float u, v, ur, view_cos, dist; /* mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos, |P - Ow| */
    int32_t level;                  /* mnTrackScaleLevel / nPredictedLevel, -1 if rejected */
    int32_t visible;                /* mbTrackInView */
} orbm_projected_point;
int orbm_project_points(int mode, const float *mp_pos, const float *mp_normal, const float *mp_min_distance,
                        const float *mp_max_distance, int m, const float *Rcw, const float *tcw, const float *Ow,
                        const orbm_camera *cam, float mbf, float viewing_cos_limit, float log_scale_factor,
                        const float *scale_factors, int nlevels, float th, orbm_projected_point *out, orbm_window_query *queries);

/* Inner loop of ORBmatcher::SearchForTriangulation (ORBmatcher.cc:892-990) with
 * CheckDistEpipolarLine (:341-358): per keypoint of KF1 (skipped if it owns a
 * MapPoint, or is mono while only_stereo), scan its BoW-node candidates of KF2 in
 * member order (CSR lists built by the host-side FeatureVector co-iteration):
 * dist <= TH_LOW && dist <= bestDist (non-strict), epipole distance^2 >=
 * 100*scaleFactor[octave2] unless one side is stereo, epipolar line d^2 <
 * 3.84*sigma2[octave2].  F12 row-major 3x3 float (LocalMapping::ComputeF12),
 * (ex, ey) the epipole in image 2.  match12[i] = index in KF2 or -1; best_dist[i].
 * The rotation histogram and the pair list stay on the host (ORBmatcher.cc:992-1023). */
int orbm_match_triangulation(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbx_keypoint *kps2,
                             const uint8_t *desc2, int n2, const int32_t *cand_off, const int32_t *cand_idx,
                             const uint8_t *has_mappoint1, const uint8_t *has_mappoint2, const uint8_t *stereo1,
                             const uint8_t *stereo2, int only_stereo, const float *F12, float ex, float ey,
                             const float *scale_factors2, const float *level_sigma2, int nlevels, int32_t *match12,
                             int32_t *best_dist);

/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:858-1024) as a whole: the FeatureVector co-iteration (:881-891,
 * :1004-1012; a FeatureVector = nodes ascending, off[nn + 1], items, as for orbm_search_by_bow), the gated loop above, the
 * rotation histogram + ComputeThreeMaxima + rejection when check_orientation (:992-1012).  match12[n1] = index in KF2 or
 * -1; vMatchedPairs = its non-negative entries in index order (:1014-1021); *nmatches = their number. */
int orbm_search_for_triangulation(const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const int32_t *nodes1, const int32_t *off1,
                                  const int32_t *items1, int nn1, const uint8_t *has_mappoint1, const uint8_t *stereo1,
                                  const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const int32_t *nodes2, const int32_t *off2,
                                  const int32_t *items2, int nn2, const uint8_t *has_mappoint2, const uint8_t *stereo2, int only_stereo,
                                  const float *F12, float ex, float ey, const float *scale_factors2, const float *level_sigma2, int nlevels,
                                  int check_orientation, int32_t *match12, int *nmatches);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:305-370) for a batch of m
 * map points: the observed descriptors of point i are rows off[i]..off[i+1) of desc
 * (bad keyframes already filtered by the caller, :325-331); best[i] = index (within
 * the point's rows) of the descriptor with the least median Hamming distance to the
 * others, first on ties, median = sorted row [int(0.5*(N-1))]; -1 if the point has
 * none.  At most 65,535 observations per point (above 128 a slower row-by-row path). */
int orbm_distinctive_descriptors(const uint8_t *desc, const int32_t *off, int m, int32_t *best);

/* DBoW2 vocabulary-tree descent = the Hamming-heavy half of Frame::ComputeBoW
 * (src/Frame.cc:410-417 -> TemplatedVocabulary::transform, Thirdparty/DBoW2/DBoW2/
 * TemplatedVocabulary.h:1127-1160 batch, :1218-1262 descent; FORB::distance,
 * FORB.cpp:81-101).  The tree is given flat: children of node i =
 * child_ids[child_off[i] .. child_off[i+1]) (node 0 = root), node_desc[nnodes][32],
 * node_word[i] = word id of a leaf (-1 inside), node_weight[i] = its idf weight;
 * L = tree depth (m_L).  transform returns, per feature, the word id, the node at
 * level L - levelsup (the FeatureVector key) and the word weight; BowVector /
 * FeatureVector (std::map insertions, addWeight in feature order, L1 normalise)
 * stay on the host.  The batch form reads descriptor sets resident in HBM
 * (orbx_result_dev layout) and leaves its outputs there; a count outside [0, cap] is clamped, rows past a set's count are
 * not written, and nsets is at most ORBM_MAX_GRID_Y = 65,535 (more: ORBX_ERR_UNSUPPORTED, nothing queued). */
typedef struct orbm_vocabulary orbm_vocabulary;
int orbm_vocab_create(const int32_t *child_off, const int32_t *child_ids, const uint8_t *node_desc, const int32_t *node_word,
                      const double *node_weight, int nnodes, int L, orbm_vocabulary **out);
int orbm_vocab_destroy(orbm_vocabulary *v);
int orbm_bow_transform(orbm_vocabulary *v, const uint8_t *features, int n, int levelsup, int32_t *word_id, int32_t *node_id,
                       double *weight);
int orbm_bow_transform_batch_dev(orbm_vocabulary *v, const uint8_t *desc_dev, const int32_t *counts_dev, int cap, int nsets,
                                 int levelsup, int32_t *word_id_dev, int32_t *node_id_dev, void *stream);

/* Acceptance test of ORBmatcher.cc:674-676: best<=th && best<(float)second*nnratio.
 * match12[i] = idx or -1; *nmatches = accepted rows.  Host arrays. */
int orbm_match_filter(int nA, const int32_t *best, const int32_t *second, const int32_t *idx,
                      int th, float nnratio, int32_t *match12, int *nmatches);

/* Batched device form used by the frames/s pipeline: descriptor sets
 * desc_dev[nsets][cap][32] with counts_dev[nsets]; pair p matches set qa[p]
 * (queries) against set qb[p].  Outputs (device): best/second/idx/match12
 * [npairs][cap] int32, nmatch[npairs]; npairs is at most ORBM_MAX_GRID_Y = 65,535 (more: ORBX_ERR_UNSUPPORTED, nothing
 * queued, nmatch not cleared).  Asynchronous on `stream`.  When the sets come straight from
 * orbx_extract_batch_dev, give both calls the SAME non-NULL stream (or synchronise between them): with NULL the
 * extractor works on its handle's stream and this call on the default stream, and nothing orders the next
 * extraction on that handle behind a match that still reads its descriptors. */
int orbm_match_batch_dev(const uint8_t *desc_dev, const int32_t *counts_dev, int cap,
                         const int32_t *pair_a_dev, const int32_t *pair_b_dev, int npairs,
                         int th, float nnratio,
                         int32_t *best_dev, int32_t *second_dev, int32_t *idx_dev,
                         int32_t *match12_dev, int32_t *nmatch_dev, void *stream);

/* Frame::AssignFeaturesToGrid (src/Frame.cc:245-260, PosInGrid :397-407) as the whole-loop searches lay a frame out: the
 * keypoints that fall inside the 64 x 48 grid (and are not skipped), ordered by (cell = col * 48 + row, keypoint index) --
 * the order in which GetFeaturesInArea visits a window.  Host only, no device call (introspection / test aid: the CPU
 * tests and the host sanitizer build check the counting sort through it).  perm[n] (first *nsorted entries valid),
 * cell_off[64 * 48 + 1]; both may be NULL. */
int orbm_sorted_frame(const orbx_keypoint *kps, int n, const uint8_t *skip, const float *uright, float min_x, float min_y,
                      float max_x, float max_y, int32_t *perm, int32_t *cell_off, int32_t *nsorted);

/* ------------------------------------------------------------------ resident frames
 * A Frame / KeyFrame as the searches need it, kept in HBM between calls: Frame::AssignFeaturesToGrid (src/Frame.cc:245-260)
 * runs once, on the device, when the handle is made -- as the reference builds mGrid once in the Frame constructor -- and
 * every search of that frame (Tracking::TrackWithMotionModel calls SearchByProjection twice, then SearchLocalPoints;
 * src/Tracking.cc) reads the same sorted keypoints, descriptors and cell table.  kps = mvKeysUn, desc = mDescriptors,
 * uright = mvuRight (NULL: monocular, all -1), (min_x .. max_y) = mnMinX .. mnMaxY.  At most 8,192 keypoints.
 * orbm_frame_from_extractor takes keypoints and descriptors of frame `frame` of the extractor's last call where they are, in
 * HBM (no trip over PCIe): xy_undistorted (n x 2 floats, or NULL when the camera has no distortion: mvKeysUn = mvKeys,
 * Frame.cc:270-275) replaces the keypoint coordinates, uright comes from the host or, with uright_from_stereo, from the
 * last orbx_stereo_match on this (left) handle (ORBX_ERR_ARG when a new frame size came since: see orbx_stereo_match).  A handle is immutable and may be searched from several threads at once;
 * what changes between calls (which keypoints already hold a map point) is an argument of each search. */
typedef struct orbm_frame orbm_frame;
int orbm_frame_create(const orbx_keypoint *kps, const uint8_t *desc, int n, const float *uright, float min_x, float min_y,
                      float max_x, float max_y, orbm_frame **out);
int orbm_frame_from_extractor(orbx_extractor *ex, int frame, const float *xy_undistorted, const float *uright, int uright_from_stereo,
                              float min_x, float min_y, float max_x, float max_y, orbm_frame **out);
int orbm_frame_destroy(orbm_frame *frame);
/* A second handle on the same device data whose SEARCHES use other bounds: a KeyFrame keeps the Frame's grid (mGrid and
 * mfGridElementWidthInv / HeightInv are copied, src/KeyFrame.cc:36) but stores mnMinX .. mnMaxY as int (include/KeyFrame.h:201-204), and
 * KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:613-657) compute with those -- on a camera with distortion the Frame's
 * bounds are fractional and the two differ.  The KeyFrame made from a Frame takes orbm_frame_alias(frame, (int)mnMinX, ...); no copy,
 * no device work; either handle may be destroyed first. */
int orbm_frame_alias(const orbm_frame *frame, float min_x, float min_y, float max_x, float max_y, orbm_frame **out);
/* n = keypoints, nsorted = those inside the grid */
int orbm_frame_size(const orbm_frame *frame, int *n, int *nsorted);
/* introspection (tests): the device-built order as orbm_sorted_frame returns it: perm[nsorted], cell_off[64 * 48 + 1] */
int orbm_frame_layout(const orbm_frame *frame, int32_t *perm, int32_t *cell_off);

/* ---- Frame::UndistortKeyPoints / ComputeImageBounds (src/Frame.cc:419-479) and frames straight from the extractor.
 * The camera as the launch files give it: mK (fx, fy, cx, cy) and mDistCoef (k1, k2, p1, p2, k3; k3 = 0 when the file has four
 * entries).  A keypoint goes through cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) as OpenCV 3.4 evaluates it for
 * CV_32FC2 points (double arithmetic, five iterations; restated in csrc/orbm_undistort.h, parity unpinned); k1 == 0 means no
 * undistortion at all, whatever the other coefficients are (the reference tests k1 only).  Near the border of a wide-angle image
 * the five iterations diverge: such results are huge or not finite, as the reference's are, and lie outside the grid.
 * Every entry refuses (ORBX_ERR_ARG) a camera with a non-finite field or with fx == 0 or fy == 0. */
typedef struct orbm_distortion { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } orbm_distortion;

/* Frame::ComputeImageBounds: bounds[4] = mnMinX, mnMinY, mnMaxX, mnMaxY (k1 == 0: 0, 0, width, height).  Host only, no device needed. */
int orbm_image_bounds(const orbm_distortion *cam, int width, int height, float *bounds);

/* n points on the device, one launch, one wait; xy / xy_un [n][2], may alias; n = 0 ok */
int orbm_undistort_points(const orbm_distortion *cam, const float *xy, int n, float *xy_un);

/* As orbm_frame_from_extractor, with the undistortion done inside the frame build: the keypoints never leave the device.  Without a
 * host uright array the call does not read the keypoint count back first (one host wait); with one it does (two).
 * cam NULL or cam->k1 == 0: exactly orbm_frame_from_extractor with xy_undistorted = NULL. */
int orbm_frame_from_extractor_cam(orbx_extractor *ex, int frame, const orbm_distortion *cam, const float *uright, int uright_from_stereo,
                                  float min_x, float min_y, float max_x, float max_y, orbm_frame **out);

/* Frames first .. first + count - 1 of the extractor's last batch -> out[0 .. count - 1]: ONE launch (a workgroup per frame), one
 * copy of every header and permutation, one host wait.  out[i] equals the single call for frame first + i.  Right coordinates come
 * from the last orbx_stereo_match (uright_from_stereo) or not at all.  All or nothing: on any failure no handle is left and out
 * is not written.  count = 0: ORBX_OK, nothing launched. */
int orbm_frames_from_extractor(orbx_extractor *ex, int first, int count, const orbm_distortion *cam, int uright_from_stereo,
                               float min_x, float min_y, float max_x, float max_y, orbm_frame **out);

/* mvKeysUn coordinates of a handle by keypoint index, xy[n][2] (what the searches use) */
int orbm_frame_keypoints_un(const orbm_frame *frame, float *xy);

/* host waits (stream synchronisations) of the last frame-making call of this process */
int orbm_debug_last_frame_build_waits(void);

/* The host-array searches above, on a resident frame (same results; `skip` / `occupied` by keypoint index as there). */
int orbm_frame_search_window(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, int nq, const uint8_t *skip,
                             int init_dist, int32_t *best, int32_t *best_level, int32_t *second, int32_t *second_level, int32_t *idx);
int orbm_frame_search_fuse(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, int nq,
                           const float *inv_level_sigma2, int nlevels, int32_t *best, int32_t *idx);
int orbm_frame_search_projection(const orbm_frame *frame, const orbm_window_query *queries, const uint8_t *qdesc, const float *qangle,
                                 const uint8_t *qtakes, int nq, const uint8_t *occupied, int th_accept, float nnratio, int ratio_same_level,
                                 int check_orientation, int32_t *match_kp, int32_t *match_q, int *nmatches);
int orbm_frame_search_for_initialization(const orbm_frame *frame2, const orbx_keypoint *kps2, const orbx_keypoint *kps1, const uint8_t *desc1,
                                         int n1, float *prev_matched, int window_size, float nnratio, int check_orientation,
                                         int32_t *matches12, int *nmatches);
int orbm_frame_search_by_projection_map(const orbm_frame *frame, const uint8_t *has_mappoint, const float *mp_pos, const float *mp_normal,
                                        const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, int m, const double *Rcw,
                                        const double *tcw, const orbm_camera *cam, const float *scale_factors, int nlevels, float th,
                                        float nnratio, int th_reloc, int32_t *matched_mp, int *nmatches, float *proj);

/* orbm_search_by_bow on two resident frames: descriptors and angles stay in HBM -- the first frame's queries are gathered on the
 * device, the second frame's features are addressed by index whether they lie inside its grid or not -- and the call uploads the
 * feature-vector lists only.  The frames' keypoint counts stand for n1 / n2 (valid1[n1], valid2[n2] or NULL, match12[n1],
 * match21[n2] or NULL); arguments and results otherwise as for orbm_search_by_bow. */
int orbm_frame_search_by_bow(const orbm_frame *frame1, const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1,
                             const uint8_t *valid1, const orbm_frame *frame2, const int32_t *nodes2, const int32_t *off2,
                             const int32_t *items2, int nn2, const uint8_t *valid2, int th, int strict_th, float nnratio,
                             int check_orientation, int32_t *match12, int32_t *match21, int *nmatches);

/* K searches of orbm_frame_search_by_bow in one call: the loop over the candidate keyframes that opens Tracking::Relocalization
 * (src/Tracking.cc:1768-1795: frame2 = the current frame in every pair, valid2 = NULL) and LoopClosing::ComputeSim3
 * (src/LoopClosing.cc:252-280: frame1 = the current keyframe in every pair).  A pair's fields are that function's arguments, and
 * pair k's match12, match21 and nmatches[k] are exactly what it returns for the pair alone, the -1 presets included.  Frames are
 * only read: the same frame may stand in any number of pairs, on either side.
 * K = 0 .. 64 (more: ORBX_ERR_UNSUPPORTED; K = 0: ORBX_OK, nothing is launched).  Every pair is checked as the single call
 * checks it, and a pair that fails fails the whole call (ORBX_ERR_ARG, ORBX_ERR_CAPACITY) before anything is launched or written.
 * One lease, one staged upload, one launch per phase (list fill; one resolver workgroup per pair) and ONE host wait for all pairs
 * that have a query; a pair without one (no common node, no valid query, an empty frame) keeps its -1 rows and takes no part.  A
 * pair whose fixed point does not settle is repeated alone on the sequential resolver, at one more wait each; the others'
 * results stand.  Under orbm_debug_force_sequential_resolver(1) every pair with a query takes that path.  Re-entrant. */
typedef struct orbm_bow_pair {
    const orbm_frame *frame1; const int32_t *nodes1, *off1, *items1; int32_t nn1; const uint8_t *valid1;   /* [frame1->n] */
    const orbm_frame *frame2; const int32_t *nodes2, *off2, *items2; int32_t nn2; const uint8_t *valid2;   /* [frame2->n] or NULL (Frame form) */
    int32_t *match12;   /* out, [frame1->n] */
    int32_t *match21;   /* out, [frame2->n], may be NULL */
} orbm_bow_pair;
int orbm_frame_search_by_bow_pairs(const orbm_bow_pair *pairs, int K, int th, int strict_th, float nnratio, int check_orientation,
                                   int32_t *nmatches /* [K] */);
/* Host waits (stream synchronisations) of the last orbm_frame_search_by_bow_pairs of this process: 0 when no pair had a query, 1
 * on the common path, one more for every pair that was repeated on the sequential resolver. */
int orbm_debug_last_bow_pairs_waits(void);

/* ORBmatcher::Fuse against K target keyframes in one call: the device half (projection block src/ORBmatcher.cc:1053-1094, gated
 * candidate loop :1092-1150; sim3 != 0: the Sim3 form, :1212-1277) of the loops LocalMapping::SearchInNeighbors
 * (src/LocalMapping.cc:550-558) and LoopClosing::SearchAndFuse (src/LoopClosing.cc:587-613) run call by call over ONE list of m
 * map points.  Row k of best / idx / projected ([K][m]) is exactly what orbm_project_points(sim3 ? ORBM_PROJECT_FUSE_SIM3 :
 * ORBM_PROJECT_FUSE, ...) followed by orbm_frame_search_fuse(targets[k].frame, ...) return for target k alone, integer for integer
 * and float bit for float bit; a rejected point has best 256, idx -1 and visible 0.  With sim3 set there is no reprojection gate
 * (as inv_level_sigma2 = NULL in the single call) and inv_level_sigma2 may be NULL.  One pyramid (scale_factors,
 * inv_level_sigma2, nlevels, log_scale_factor) and one th serve all targets.
 * active ([K][m] bytes, or NULL = all ones): active[k][i] == 0 says the caller knows the loop skips this pair (a NULL entry, a bad
 * point, a point already in keyframe k, a point in spAlreadyFound); its row entries are the presets 256, -1 and the rejected
 * record (visible 0, level -1), and it does no work on the device.
 * K = 0 .. 128, m = 0 .. 65,536, K * m <= 4,194,304 (beyond: ORBX_ERR_UNSUPPORTED).  K = 0, m = 0 or no active pair: ORBX_OK,
 * nothing is launched, 0 waits.  Every target is checked as the single calls check theirs -- a frame, a finite pose, with the
 * gate on every octave of the frame in [0, nlevels), nlevels 1 .. 16 -- and one that fails fails the whole call (ORBX_ERR_ARG)
 * before anything is launched or written.  Frames are only read; the same frame may stand in several targets.  A launching call
 * takes one lease, one staged upload, one launch and ONE host wait.  Re-entrant.
 * The map update stays with the caller, target by target in list order; MapPoint::Replace recomputes the heir's descriptor, so
 * the rows of later targets for such entries are refreshed by one more call (orbslam_hip.hpp: ORBmatcher::FuseKeyFrames). */
typedef struct orbm_fuse_target {
    const orbm_frame *frame;          /* resident keyframe (mvKeysUn, mvuRight, descriptors, grid) */
    float Rcw[9], tcw[3], Ow[3];      /* as orbm_project_points takes them; Sim3 form: sRcw / s, t / s, -Rcw' tcw (:1188-1192) */
    orbm_camera cam;                  /* fx .. cy, image bounds (KeyFrame::IsInImage), grid bounds */
    float mbf;
} orbm_fuse_target;
int orbm_fuse_keyframes(const orbm_fuse_target *targets, int K, int sim3, const float *mp_pos, const float *mp_normal,
                        const float *mp_min_distance, const float *mp_max_distance, const uint8_t *mp_desc, int m,
                        const uint8_t *active /* [K][m] or NULL */, float th, float log_scale_factor, const float *scale_factors,
                        const float *inv_level_sigma2, int nlevels, int32_t *best /* [K][m] */, int32_t *idx /* [K][m] */,
                        orbm_projected_point *projected /* [K][m] or NULL */);
/* Host waits (stream synchronisations) of the last orbm_fuse_keyframes of this process: 1 when it launched, else 0. */
int orbm_debug_last_fuse_keyframes_waits(void);

/* orbm_search_for_triangulation on two resident keyframes: a keypoint is "stereo" where the frame's right coordinate is >= 0
 * (mvuRight, as given to orbm_frame_create / taken from ComputeStereoMatches); the call uploads the feature-vector lists and the two
 * "owns a MapPoint" masks, and the rotation histogram runs on angle differences formed on the device.  Positions are the frames'
 * (mvKeysUn) coordinates.  has_mappoint1[n1], has_mappoint2[n2], match12[n1]; otherwise as orbm_search_for_triangulation. */
int orbm_frame_search_for_triangulation(const orbm_frame *kf1, const int32_t *nodes1, const int32_t *off1, const int32_t *items1, int nn1,
                                        const uint8_t *has_mappoint1, const orbm_frame *kf2, const int32_t *nodes2, const int32_t *off2,
                                        const int32_t *items2, int nn2, const uint8_t *has_mappoint2, int only_stereo, const float *F12,
                                        float ex, float ey, const float *scale_factors2, const float *level_sigma2, int nlevels,
                                        int check_orientation, int32_t *match12, int *nmatches);

/* ------------------------------------------- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:243-520) in one call
 * The loop over the neighbour keyframes -- SearchForTriangulation(cur, neighbour, F12, .., false) chained into the parallax test,
 * the linear triangulation (cv::SVD) or UnprojectStereo, the depth tests, the two reprojection gates and the scale-consistency
 * gate -- for all K neighbours in ONE launch, one upload and one host wait.  What one neighbour hands to the next is only "this
 * keypoint of the current keyframe owns a point now" (ORBmatcher.cc:900-904); the device carries it from k to k + 1.
 *
 * The caller passes the neighbours that passed the baseline test of :288-308 (it needs ComputeSceneMedianDepth, a walk over the
 * map), in the order of GetBestCovisibilityKeyFrames, each with its F12 (LocalMapping::ComputeF12) and the epipole (ex, ey) as for
 * orbm_frame_search_for_triangulation.  One pyramid (scale_factors, level_sigma2 [nlevels], scale_factor = mfScaleFactor) serves
 * all keyframes: a map's keyframes share the extractor.  With the caller stay new MapPoint, AddObservation, AddMapPoint,
 * ComputeDistinctiveDescriptors, UpdateNormalAndDepth -- to be replayed over the results in (k, i) ascending order, the
 * reference's creation order -- and the CheckNewKeyFrames() early return between neighbours (:283): one call cannot be
 * interrupted, so a caller that needs the early return calls with the neighbours in chunks, updating has_mappoint of the current
 * keyframe from the results in between.
 *
 * Positions are the frames' (mvKeysUn) coordinates, also in UnprojectStereo (which reads mvKeys: the same for rectified stereo;
 * for an RGB-D camera with distortion they differ).  A stereo keypoint (uright >= 0) whose depth is not > 0, where the reference
 * cannot go on, is rejected as ORBM_TRI_PARALLAX. */
typedef struct orbm_triang_keyframe {
    const orbm_frame *frame;        /* mvKeysUn / mvuRight / descriptors resident (at most 8,192 keypoints) */
    const float *Tcw;               /* 4 x 4 row-major, as cv::Mat mTcw */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    const float *depth;             /* mvDepth[n]; NULL only if no keypoint of the frame has uright >= 0 (a frame made from device arrays with right coordinates always needs it) */
    const uint8_t *has_mappoint;    /* [n]: GetMapPoint(i) != NULL before the call */
    const int32_t *nodes, *off, *items; int32_t nn;   /* mFeatVec, flat as for orbm_search_by_bow */
    const float *F12; float ex, ey; /* neighbours only: LocalMapping::ComputeF12 and the epipole, computed by the caller */
} orbm_triang_keyframe;

/* What became of keypoint i of the current keyframe against neighbour k.  The reference's counters: nTriangulationRejects =
 * SVD_ZERO, nParalaxRejects = PARALLAX, nDepthRejects = DEPTH, nRepErrorRejects = REPROJ1 (:465 / :476 count nothing),
 * nScaleConsRejects = SCALE, each summed over k. */
enum { ORBM_TRI_NO_MATCH = -1, ORBM_TRI_CREATED = 0, ORBM_TRI_SKIPPED = 1 /* owns a point */, ORBM_TRI_SVD_ZERO = 2,
       ORBM_TRI_PARALLAX = 3, ORBM_TRI_DEPTH = 4, ORBM_TRI_REPROJ1 = 5, ORBM_TRI_REPROJ2 = 6, ORBM_TRI_DIST_ZERO = 7,
       ORBM_TRI_SCALE = 8, ORBM_TRI_NSTATUS = 9 };

/* K = 0 .. 32 neighbours (more: ORBX_ERR_UNSUPPORTED; K = 0 or an empty current keyframe: ORBX_OK, *nnew = 0, nothing is
 * launched).  An octave outside [0, nlevels) in any frame, or depth = NULL on a frame with a stereo keypoint, is
 * ORBX_ERR_ARG before the launch.  Results by keypoint index i of the current keyframe (n1 of them), row k per neighbour:
 *   match12[k][i]   keypoint of neighbour k the search gave i, or -1
 *   status[k][i]    ORBM_TRI_*
 *   x3d[k][i][3]    the new point, written ONLY where status[k][i] == ORBM_TRI_CREATED
 *   counts[k][s]    (optional) how many i have status s = 0 .. 8, [K][ORBM_TRI_NSTATUS]
 *   *nnew           number of points created = the reference's nnew. */
int orbm_create_new_map_points(const orbm_triang_keyframe *cur, const orbm_triang_keyframe *neigh, int K,
                               const float *scale_factors, const float *level_sigma2, int nlevels, float scale_factor,
                               int32_t *match12, int8_t *status, float *x3d, int32_t *counts, int *nnew);
/* Host waits (stream synchronisations) of the last orbm_create_new_map_points call of this process: 1 when it launched, 0 when it
 * returned before the launch. */
int orbm_debug_last_create_points_waits(void);

/* ------------------------------------------- Sim3Solver: every RANSAC hypothesis of a loop detection in one call
 * Sim3Solver::iterate (src/Sim3Solver.cc:140-207) draws three indices per iteration from a freshly reset list (:163-177), so no
 * iteration depends on an earlier one: the caller draws the triples of all iterations first, this call evaluates ComputeSim3
 * (:226-337) and CheckInliers (:340-364) for each, and what iterate returns is a fold over the inlier counts that the caller runs
 * on the host (include/orbslam_hip.hpp: Sim3Solver).  One problem per candidate keyframe; the pointer walk of the constructor
 * (:62-103) stays with the caller, who passes what it keeps, flat. */
typedef struct orbm_sim3_problem {
    const float *X1w, *X2w;            /* [n][3] world positions of the pairs the constructor keeps (:64-101), in that order */
    const int32_t *octave1, *octave2;  /* [n] kp.octave of the two keypoints */
    const float *Tcw1, *Tcw2;          /* 4 x 4 row-major */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    const int32_t *triples;            /* [H][3] indices into 0..n-1 as the draw loop :166-177 leaves them */
    int32_t n, H, fix_scale;
} orbm_sim3_problem;

typedef struct orbm_sim3_hypothesis {
    float T12[16], R12[9], t12[3], s12; /* mT12i, mR12i, mt12i, ms12i of the hypothesis */
    int32_t ninliers;                   /* mnInliersi */
} orbm_sim3_hypothesis;

/* P = 0 .. 64 problems, n <= 8,192 correspondences and H <= 1,024 hypotheses each (beyond: ORBX_ERR_UNSUPPORTED).  P = 0, or H = 0
 * in every problem: ORBX_OK, nothing is launched.  ORBX_ERR_ARG before the launch: n < 3 with H > 0, a triple index outside
 * [0, n), a triple that repeats an index, an octave outside [0, nlevels).  level_sigma2 [nlevels] = mvLevelSigma2 (one pyramid: a
 * map's keyframes share the extractor).
 *   hyp[sum H]   the hypotheses of problem 0, then of problem 1, ...
 *   inliers      (void *: the binder maps no uint64_t pointer of its own; the words are uint64_t) per problem, behind each other,
 *                [H][(n + 63) / 64] 64-bit words: bit i % 64 of word i / 64 = mvbInliersi[i]; bits past n are 0.
 * There is no depth test in Project (:382-403): a correspondence with z <= 0 is projected like any other, and a NaN position is
 * never an inlier.  The exact identity rotation gives NaN throughout, as the reference's 0 / 0 at :280 does: 0 inliers. */
int orbm_sim3_hypotheses(const orbm_sim3_problem *problems, int P, const float *level_sigma2, int nlevels,
                         orbm_sim3_hypothesis *hyp, void *inliers);
/* Host waits (stream synchronisations) of the last orbm_sim3_hypotheses call of this process: 1 when it launched, 0 when it
 * returned before the launch. */
int orbm_debug_last_sim3_waits(void);

/* ------------------------------------------- PnPsolver: every EPnP RANSAC hypothesis of a relocalisation in one call
 * PnPsolver::iterate (src/PnPsolver.cc:170-263) draws four indices per iteration from a freshly reset list (:193-206), so no
 * iteration depends on an earlier one: the caller draws the sets of all iterations first, this call evaluates compute_pose
 * (:938-986) and CheckInliers (:763-794) for each, runs Refine (:649-694) behind every hypothesis that sets a new best, and what
 * iterate returns is a fold over the results that the caller runs on the host (include/orbslam_hip.hpp: PnPsolver).  One problem
 * per candidate keyframe; the pointer walk of the constructor (:81-103) stays with the caller, who passes what it keeps, flat.
 * All of EPnP is IEEE double with one stated departure from the reference (its SVD's std::hypot). */
typedef struct orbm_pnp_problem {
    const float *Xw;          /* [n][3] mvP3Dw, in the constructor's order (:81-103) */
    const float *uv;          /* [n][2] mvP2D */
    const int32_t *octave;    /* [n] kp.octave -> mvSigma2 */
    const int32_t *sets;      /* [H][4] indices into 0..n-1 as the draw loop leaves them */
    double fu, fv, uc, vc;
    float th2;                /* 5.991 */
    int32_t n, H, min_inliers;/* mRansacMinInliers AFTER SetRansacParameters */
} orbm_pnp_problem;

typedef struct orbm_pnp_hypothesis {
    double R[9], t[3], rep_error;  /* mRi, mti, compute_pose's return */
    int32_t ninliers;              /* mnInliersi */
    int32_t refined;               /* 1: this hypothesis set a new best with >= min_inliers, Refine() ran on ITS inliers */
    double Rr[9], tr[3];           /* Refine's mRi, mti   (refined == 1; else 0) */
    int32_t nrefined, pad;         /* mnRefinedInliers    (refined == 1; else 0) */
} orbm_pnp_hypothesis;

/* P = 0 .. 64 problems, n <= 8,192 correspondences and H <= 1,024 hypotheses each (beyond: ORBX_ERR_UNSUPPORTED).  P = 0, or H = 0
 * in every problem: ORBX_OK, nothing is launched.  ORBX_ERR_ARG before the launch: n < 4 with H > 0, a set index outside [0, n),
 * an octave outside [0, nlevels), min_inliers < 1.  A set MAY repeat an index (the second iterate of the reference erases the
 * wrong element of its draw list, :315); EPnP of a repeated correspondence is well defined.  level_sigma2 [nlevels] =
 * mvLevelSigma2.  best_in [P] = mnBestInliers as the solvers carry it into the call (NULL: 0 for all).
 *   hyp[sum H]        the hypotheses of problem 0, then of problem 1, ...  Within a problem, in order, a hypothesis with
 *                     ninliers >= min_inliers and ninliers > the running best (which starts at best_in) is a record: refined = 1,
 *                     and Rr, tr, nrefined are what Refine() computes from its inliers.  The reference also calls Refine() behind
 *                     hypotheses that reach min_inliers without a record: those repeat the previous computation on an unchanged
 *                     mvbBestInliers and return the same false.  Records behind the one whose Refine succeeds are speculative.
 *   inliers           (void *: the words are uint64_t) per problem, behind each other, [H][(n + 63) / 64] 64-bit words: bit i % 64
 *                     of word i / 64 = mvbInliersi[i]; bits past n are 0.
 *   refined_inliers   the same layout: mvbRefinedInliers of a record, 0 for every other hypothesis.
 * A Refine set may hold all n correspondences.  A NaN coordinate is never an inlier. */
int orbm_pnp_hypotheses(const orbm_pnp_problem *problems, int P, const float *level_sigma2, int nlevels, const int32_t *best_in,
                        orbm_pnp_hypothesis *hyp, void *inliers, void *refined_inliers);
/* Host waits (stream synchronisations) of the last orbm_pnp_hypotheses call of this process: 1 when it launched, 0 when it
 * returned before the launch. */
int orbm_debug_last_pnp_waits(void);
/* compute_pose (:938-986) of n = 4 .. 2,048 correspondences in double (pws [n][3], us [n][2]) on the HOST, through the same header
 * the kernels instantiate; needs no device (test aid).  R [9] row-major, t [3], *rep_error = its return value. */
int orbm_debug_pnp_pose(const double *pws, const double *us, int n, const double *fu_fv_uc_vc, double *R, double *t, double *rep_error);

/* ------------------------------------------- Optimizer::OptimizeSim3: the loop-closing Sim3 refinement in one call
 * The whole of src/Optimizer.cc:1564-1624 -- optimize(5), the outlier cut, optimize(5 or 10), the final count -- for up to 64 loop
 * candidates in ONE launch, on g2o's code paths (VertexSim3Expmap, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ with g2o's numeric
 * Jacobians, Levenberg, the dense LDLT solver, the Huber kernel).  The pointer walk of :1483-1520 stays with the caller,
 * who passes the correspondences it keeps, flat and in that order. */
typedef struct orbm_sim3_opt_problem {
    const float *X1w, *X2w;            /* [n][3] GetWorldPos() of pMP1 / pMP2 */
    const float *obs1, *obs2;          /* [n][2] mvKeysUn[i].pt of pKF1, mvKeysUn[i2].pt of pKF2 */
    const int32_t *octave1, *octave2;  /* [n] the two keypoints' octaves */
    const float *Tcw1, *Tcw2;          /* 4 x 4 row-major: R1w, t1w, R2w, t2w */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float R12[9], t12[3], s12;         /* the Sim3 as LoopClosing.cc:320-325 hands it over (Sim3(Matrix3d, Vector3d, double)) */
    float th2;
    int32_t fix_scale, n;
} orbm_sim3_opt_problem;

typedef struct orbm_sim3_opt_result {
    double q[4], t[3], s;               /* g2oS12 on return: rotation x y z w, translation, scale (the input when nin is :1596's 0) */
    int32_t nin;                        /* the return value */
    int32_t nbad, ncorrespondences;     /* nBad of the first cut, nCorrespondences */
    int32_t iterations[2], trials[2];   /* test aids: Levenberg iterations and damped solves of the two optimize() calls */
    double chi2;                        /* currentChi after the last iteration run (0 if none) */
} orbm_sim3_opt_result;

/* P = 0 .. 64 problems, n <= 8,192 correspondences each (beyond: ORBX_ERR_UNSUPPORTED).  P = 0, or n = 0 in every problem: ORBX_OK,
 * nothing is launched (results are still filled: the input Sim3, nin = 0).  An octave outside [0, nlevels): ORBX_ERR_ARG before the
 * launch.  inv_level_sigma2 [nlevels] = mvInvLevelSigma2 (one pyramid: a map's keyframes share the extractor).
 *   results[P]
 *   kept         the problems behind each other, [n] each: 1 where the reference leaves vpMatches1[idx] non-NULL.  When fewer than
 *                10 pairs survive the first cut (:1595) the cut is applied, nin = 0 and the Sim3 is the input.
 * A NaN position makes every sum NaN: no step is accepted, no chi2 is > th2, every pair is kept and counted, as in the reference. */
int orbm_optimize_sim3(const orbm_sim3_opt_problem *problems, int P, const float *inv_level_sigma2, int nlevels,
                       orbm_sim3_opt_result *results, uint8_t *kept);
/* Host waits (stream synchronisations) of the last orbm_optimize_sim3 call of this process: 1 when it launched, 0 when it returned
 * before the launch. */
int orbm_debug_last_sim3_opt_waits(void);

/* ------------------------------------------- Initializer: every H / F hypothesis of a monocular initialisation in one call
 * Initializer::Initialize (src/Initializer.cc:44-121) draws the 8-point sets of all iterations first (:77-97); no hypothesis reads
 * another's result, and FindHomography (:124-172) / FindFundamental (:175-223) return a fold over the per-hypothesis scores.
 * orbm_init_find_models evaluates all 2 H hypotheses in ONE launch and runs both folds; orbm_init_check_rt is CheckRT (:798-907)
 * for up to 8 motions in ONE launch; orbm_init_reconstruct_f is ReconstructF (:470-570) around one orbm_init_check_rt call.
 * ReconstructH (:572-732) is NOT here: this fork takes it only at RH > 0.99 (:115), the host classes report that case as its
 * own status and the integration shell runs the reference's own ReconstructH there (its CheckRT calls go one motion at a time).
 * The OpenCV arithmetic (cv::SVDecomp, cv::invert, the 3 x 3 products) is restated from OpenCV 3.4 and unpinned.
 *
 * Shared arguments: keys1 [n1][2] / keys2 [n2][2] = mvKeysUn[i].pt of the reference and the current frame (ALL keypoints: Normalize
 * sums over every one, :749-795); matches [n][2] = mvMatches12 (index into keys1, index into keys2) in that order.  n <= 8,192
 * (beyond: ORBX_ERR_UNSUPPORTED); a match index outside its frame: ORBX_ERR_ARG. */
typedef struct orbm_init_models {
    float H21[9], F21[9];              /* the winning matrices, row-major (zeros when none won) */
    float SH, SF;                      /* their scores (0 when none won) */
    int32_t itH, itF;                  /* the winning iterations; -1 = no hypothesis scored above 0 */
} orbm_init_models;

typedef struct orbm_init_reconstruction {
    float R21[9], t21[3];              /* the motion, when found */
    float parallax[4];                 /* parallax1 .. parallax4 of the four CheckRT calls, (R1,t) (R2,t) (R1,-t) (R2,-t) */
    int32_t ngood[4];                  /* nGood1 .. nGood4 */
    int32_t found, best, N, max_good, nsimilar;   /* the return value; the motion the == cascade picked (-1: rejected before);
                                                     the inlier count N; maxGood; nsimilar */
} orbm_init_reconstruction;

/* sets [H][8] = mvSets (indices into 0..n-1), sigma = mSigma.  H <= 1,024 (beyond: ORBX_ERR_UNSUPPORTED).  ORBX_ERR_ARG before the
 * launch: a set index outside [0, n) or repeated within a set, n < 8 with H > 0, sigma <= 0.  H = 0: ORBX_OK, nothing is launched.
 *   out          the folds of :148-171 / :199-222: the first hypothesis whose score is > every earlier one, starting from 0.  A NaN
 *                score (a singular H21i inverts to zeros) and a score of exactly 0 never win.
 *   mask_h / _f  (void *: the words are uint64_t) [(n + 63) / 64]: bit i % 64 of word i / 64 = vbMatchesInliersH / F[i]; bits past n
 *                are 0.  No H winner: n falses, SH = 0, itH = -1.  No F winner: the reference leaves vbMatchesInliersF EMPTY (:178
 *                reads N from the size of the output vector) and F21 an empty cv::Mat, and ReconstructF would throw; here itF = -1,
 *                SF = 0 and the mask is zeros.
 *   hyp_*        per hypothesis, the H model's H first, then the F model's: matrices [2 H][9], scores [2 H], masks
 *                [2 H][(n + 63) / 64] uint64_t.  Each may be NULL. */
int orbm_init_find_models(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n,
                          const int32_t *sets, int H, float sigma, orbm_init_models *out, void *mask_h, void *mask_f,
                          float *hyp_matrices, float *hyp_scores, void *hyp_masks);
/* CheckRT for M <= 8 motions (beyond: ORBX_ERR_UNSUPPORTED): R [M][9], t [M][3], K 3 x 3 row-major, inliers [n] bytes =
 * vbMatchesInliers.  M = 0 launches nothing.  Per motion:
 *   good [M][n1] bytes = vbGood, P3D [M][n1][3] = vP3D (entries the reference never writes are 0; a counted match with
 *   cosParallax >= 0.9998 has its P3D written and good 0); counted [M][n], cos_parallax [M][n] per match (either may be NULL);
 *   ngood [M] = the return value; parallax [M] (0 with ngood = 0). */
int orbm_init_check_rt(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n,
                       const uint8_t *inliers, const float *K, const float *R, const float *t, int M, float th2, uint8_t *good,
                       float *P3D, uint8_t *counted, float *cos_parallax, int32_t *ngood, float *parallax);
/* ReconstructF(vbMatchesInliers, F21, K, R21, t21, vP3D, vbTriangulated, minParallax, minTriangulated): P3D [n1][3] and
 * triangulated [n1] are written when out->found, else zeros. */
int orbm_init_reconstruct_f(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int n,
                            const uint8_t *inliers, const float *F21, const float *K, float sigma, float min_parallax,
                            int min_triangulated, orbm_init_reconstruction *out, float *P3D, uint8_t *triangulated);
/* Host waits (stream synchronisations) of the last orbm_init_* call of this process: 1 when it launched, 0 when it returned
 * before the launch. */
int orbm_debug_last_init_waits(void);
/* Test aid, host only: the library's restatement of cv::SVDecomp (csrc/orbm_svd.h) on one matrix.  shape 0: A 16 x 9 -> vt [9] =
 * vt.row(8); 1: A 8 x 9 -> vt [9] = vt.row(8) (FULL_UV); 2: A 3 x 3 -> w [3], u [9], vt [9]; 3: A 4 x 4 -> vt [4] = vt.row(3). */
int orbm_debug_init_svd(int shape, const float *A, float *w, float *u, float *vt);

/* ------------------------------------------- the whole-map relocalisation search under P poses in one call
 * PnPsolver::iterate(Frame&, .., Map*) (src/PnPsolver.cc:267-646) calls SearchByProjection(F, pMap, Rcw, tcw, ..) over and over
 * with the same frame and the same map: after every refined RANSAC hypothesis (:355-398) and, in its second stage (:419-634), for
 * up to five recorded poses walked twice.  Nothing couples those searches -- the search writes no state another search reads -- so
 * all poses of a stage run in ONE launch, with one upload and one host wait.
 *
 * orbm_map is a snapshot of what pMap->GetAllMapPoints() returned: the five arrays of orbm_search_by_projection_map
 * (mp_min_dist / mp_max_dist = GetMinDistanceInvariance() / GetMaxDistanceInvariance(), 32-byte descriptors), copied to HBM once.
 * Opaque and immutable like orbm_frame: no slots, no updates, no link to orbm_points; it may be searched from several threads at
 * once.  m = 0 is legal.  One Tracking::Relocalization() makes one snapshot and uses it for every candidate keyframe. */
typedef struct orbm_map orbm_map;
int orbm_map_create(const float *mp_pos, const float *mp_normal, const float *mp_min_dist, const float *mp_max_dist,
                    const uint8_t *mp_desc, int m, orbm_map **out);
int orbm_map_destroy(orbm_map *map);
int orbm_map_size(const orbm_map *map, int *m);

/* Rcw [P][9] row-major, tcw [P][3].  Row p of every output is what orbm_frame_search_by_projection_map returns for pose p, bit for
 * bit: matched_mp [P][n] (the last map point wins), nmatches [P] (acceptances, not occupied slots), proj [P][m][4] or NULL (u, v,
 * viewCos, level; level -1 where culled).  A pose's rows do not depend on the other poses of the call or on their order.
 * has_mappoint [n] by keypoint index, or NULL: no keypoint holds a map point.
 *   P = 0, m = 0 or n = 0   ORBX_OK, rows preset (-1 / 0), nothing is launched
 *   P > 16                  ORBX_ERR_UNSUPPORTED (the second stage makes at most 10 searches)
 *   ORBX_ERR_ARG            a NULL array that is needed, P < 0, nlevels outside 1 .. 16, a keypoint octave outside 0 .. 15
 * Every refusal happens before any device work and writes nothing.  The host-array form uploads frame and map with the call. */
int orbm_frame_search_by_projection_map_poses(const orbm_frame *frame, const uint8_t *has_mappoint, const orbm_map *map,
                                              const double *Rcw, const double *tcw, int P, const orbm_camera *cam,
                                              const float *scale_factors, int nlevels, float th, float nnratio, int th_reloc,
                                              int32_t *matched_mp, int32_t *nmatches, float *proj);
int orbm_search_by_projection_map_poses(const orbx_keypoint *kps, const uint8_t *desc, int n, const uint8_t *has_mappoint,
                                        const float *mp_pos, const float *mp_normal, const float *mp_min_dist,
                                        const float *mp_max_dist, const uint8_t *mp_desc, int m, const double *Rcw,
                                        const double *tcw, int P, const orbm_camera *cam, const float *scale_factors, int nlevels,
                                        float th, float nnratio, int th_reloc, int32_t *matched_mp, int32_t *nmatches, float *proj);
/* Host waits (stream synchronisations) of the last ..._map_poses call of this process: 1 when it launched, 0 when it returned
 * before the launch. */
int orbm_debug_last_map_poses_waits(void);

/* ------------------------------------------- the SearchByProjection forms and SearchBySim3 as WHOLE functions
 * Projection prefix, candidate search, in-loop assignment, acceptance and rotation check in one call, nothing in between
 * returns to the host.  The pointer graph is passed flat: entry i of the vector the reference walks (LastFrame.mvpMapPoints,
 * pKF->GetMapPointMatches(), vpPoints) becomes
 *   valid[i]         what the reference's pointer tests leave: non-NULL and not an outlier (:1555-1558) / not bad and not in
 *                    sAlreadyFound (:1697-1700) / not bad and not in spAlreadyFound (:516-517) / non-NULL, not already
 *                    matched, not bad (:1352-1358)
 *   pos[i][3]        MapPoint::GetWorldPos          desc[i][32]   MapPoint::GetDescriptor
 *   normal[i][3]     GetNormal (Sim3 form)          min_distance / max_distance[i]   mfMinDistance / mfMaxDistance (the 0.8 /
 *                                                   1.2 of Get{Min,Max}DistanceInvariance are applied by the library)
 *   takes[i]         Observations() > 0 (Cur/Last form: :1603-1605; NULL = every assignment blocks its slot)
 *   octave[i]        LastFrame.mvKeys[i].octave (Cur/Last form)
 *   angle[i]         mvKeysUn[i].angle of the source keypoint (rotation check)
 * Arrays a form does not read may be NULL.  orbm_view = calibration + scale pyramid of the searched frame (fx .. cy, mb, mbf,
 * mfLogScaleFactor, mvScaleFactors); the image bounds are the frame handle's.  Poses are 4 x 4 row-major floats as cv::Mat
 * mTcw holds them; cv::Mat arithmetic on them (Rcw, tcw, twc, tlc, Ow, the Sim3 decomposition) is done by the library in the
 * reference's order.  occupied[j] (by keypoint index, NULL = none): the slot is taken before the call -- mvpMapPoints[j] with
 * Observations() > 0 (:1603-1605), mvpMapPoints[j] != NULL (:1741-1742), vpMatched[j] != NULL (:574-575).
 * Outputs as orbm_search_projection: match_kp[n] (entry index, -1 untouched, -2 cleared by the rotation check), match_q[entries],
 * *nmatches; queries_out (optional, test aid) = the GetFeaturesInArea query formed per entry (r < 0: skipped before the search). */
typedef struct orbm_points {
    int32_t n;
    const uint8_t *valid;
    const float *pos, *normal, *min_distance, *max_distance;
    const uint8_t *desc, *takes;
    const int32_t *octave;
    const float *angle;
} orbm_points;
typedef struct orbm_view {
    float fx, fy, cx, cy, mb, mbf, log_scale_factor;
    int32_t nlevels;
    const float *scale_factors;
} orbm_view;
/* Tracking::SearchLocalPoints' data plane (src/Tracking.cc): Frame::isInFrustum(pMP, viewing_cos_limit = 0.5) for every listed
 * point (src/Frame.cc:284-340, with MapPoint::PredictScale) chained into SearchByProjection(Frame &F, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:46-132: RadiusByViewingCos, levels [l-1, l], stereo test, best / second with levels, <= th_high = TH_HIGH,
 * ratio test on equal levels).  valid[i] = the point is not bad and was not already matched in this frame (mnLastFrameSeen);
 * takes[i] = Observations() > 0; occupied[j] = mvpMapPoints[j] holds an observed point (:87-89).  projected_out (optional) =
 * what isInFrustum leaves in the MapPoint (mbTrackInView, mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos) for the
 * caller's IncreaseVisible bookkeeping. */
int orbm_search_by_projection_points(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *points,
                                     const uint8_t *occupied, float th, float viewing_cos_limit, int th_high, float nnratio, int32_t *match_kp,
                                     int32_t *match_q, int *nmatches, orbm_projected_point *projected_out, orbm_window_query *queries_out);
/* SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)   src/ORBmatcher.cc:1529-1671
 * (th_high = TH_HIGH).  THE per-frame matcher call of Tracking::TrackWithMotionModel. */
int orbm_search_by_projection_last(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const float *Tlw, const orbm_points *last,
                                   const uint8_t *occupied, float th, int mono, int th_high, int check_orientation, int32_t *match_kp,
                                   int32_t *match_q, int *nmatches, orbm_window_query *queries_out);
/* SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)
 * src/ORBmatcher.cc:1673-1800 (relocalisation refinement). */
int orbm_search_by_projection_keyframe(const orbm_frame *cur, const orbm_view *view, const float *Tcw, const orbm_points *kf,
                                       const uint8_t *occupied, float th, int orb_dist, int check_orientation, int32_t *match_kp,
                                       int32_t *match_q, int *nmatches, orbm_window_query *queries_out);
/* SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
 * src/ORBmatcher.cc:491-604 (loop closing; th_low = TH_LOW).  Scw 4 x 4. */
int orbm_search_by_projection_sim3(const orbm_frame *kf, const orbm_view *view, const float *Scw, const orbm_points *points,
                                   const uint8_t *occupied, int th, int th_low, int32_t *match_kp, int32_t *match_q, int *nmatches,
                                   orbm_window_query *queries_out);
/* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)   src/ORBmatcher.cc:1303-1527: both projections, both window searches
 * (levels [l-1, l], best from INT_MAX, <= th_high = TH_HIGH) and the agreement check.  points1 / points2 have one entry per
 * keypoint of kf1 / kf2 (valid folds vbAlreadyMatched1 / 2 in); T1w / T2w = the key frames' poses, R12 3 x 3, t12 3.
 * vnMatch1 / vnMatch2 (optional) as the reference's locals; match12[i1] = idx2 where both directions agree, else -1 (the entries
 * of vpMatches12 the reference overwrites, :1513-1521); *nfound. */
int orbm_search_by_sim3(const orbm_frame *kf1, const orbm_frame *kf2, const orbm_view *view, const float *T1w, const float *T2w, float s12,
                        const float *R12, const float *t12, const orbm_points *points1, const orbm_points *points2, float th, int th_high,
                        int32_t *vnMatch1, int32_t *vnMatch2, int32_t *match12, int *nfound, orbm_window_query *q12_out,
                        orbm_window_query *q21_out);

/* ------------------------------------------- LoopClosing::ComputeSim3's refinement: SearchBySim3 chained into OptimizeSim3
 * src/LoopClosing.cc:311-341 for up to 64 refinement attempts against one current keyframe in ONE call: per attempt SearchBySim3
 * (src/ORBmatcher.cc:1303-1527), the correspondence walk of OptimizeSim3 (src/Optimizer.cc:1483-1520) and OptimizeSim3 itself, with
 * one staged upload and one host wait; nothing returns to the host in between.  An attempt has no side effects in the
 * reference (vpMapPointMatches and gScm are its locals), so the attempts of one pass of the loop at :288 can be evaluated together
 * and the host takes the first in order with nin >= 20.
 * Shared: kf1 = mpCurrentKF, points1 = one entry per keypoint of kf1 (valid = map point non-NULL and not bad; pos, desc,
 * min_distance, max_distance), T1w, view (fx .. cy serve both keyframes, as in orbm_search_by_sim3), inv_level_sigma2 [view->nlevels].
 * Per attempt: kf2, points2 (one entry per keypoint of kf2), T2w, the Sim3 as LoopClosing.cc:320-325 hands it over, and
 *   seed12[n1]     vpMapPointMatches as the attempt starts from it (:313-319): >= 0 the point's GetIndexInKeyFrame(pKF2), -1 NULL,
 *                  -2 non-NULL without an index in KF2 (blocks slot i1 in the search, ORBmatcher.cc:1335-1338, marks nothing in
 *                  KF2, and OptimizeSim3 skips it at Optimizer.cc:1498).  vbAlreadyMatched1 / 2 are derived from it by the library:
 *                  valid does NOT fold them in, unlike orbm_search_by_sim3.  NULL = all -1.
 *   found12[n1]    (out) match12 of orbm_search_by_sim3 alone; nfound[p] its count
 *   matches12[n1]  (out) vpMatches1 as OptimizeSim3 leaves it: seed12[i1] >= 0 ? seed12[i1] : found12[i1], set to -1 where the cut
 *                  (:1577-1590 / :1611-1620) erased it; -2 stays -2
 * results[P]: as orbm_optimize_sim3.  A pair (i1, i2 = the merged index) is a correspondence iff i2 >= 0, points1.valid[i1] and
 * points2.valid[i2]; the correspondences are optimised in ascending i1. */
typedef struct orbm_refine_sim3_attempt {
    const orbm_frame *kf2;
    const orbm_points *points2;
    const float *T2w;                  /* 4 x 4 row-major */
    float R12[9], t12[3], s12;
    const int32_t *seed12;
    int32_t *found12, *matches12;
} orbm_refine_sim3_attempt;

/* P = 0 .. 64 attempts (beyond: ORBX_ERR_UNSUPPORTED), frames of at most 8,192 keypoints.  ORBX_ERR_ARG before anything is launched,
 * with every output untouched: points.n != the handle's n, a seed >= n2 or < -2, a keypoint octave outside [0, nlevels).  P = 0, or
 * a kf1 without keypoints: ORBX_OK, nothing is launched.  An attempt whose kf2 has no keypoints returns the input Sim3 and nin = 0,
 * as orbm_optimize_sim3 does for n = 0.  th = 7.5, th_high = TH_HIGH, th2 = 10 in the reference. */
int orbm_refine_sim3_candidates(const orbm_frame *kf1, const orbm_points *points1, const float *T1w, const orbm_view *view,
                                const float *inv_level_sigma2, const orbm_refine_sim3_attempt *attempts, int P, float th, int th_high,
                                float th2, int fix_scale, int32_t *nfound, orbm_sim3_opt_result *results);
/* Host waits (stream synchronisations) of the last orbm_refine_sim3_candidates call of this process: 1 when it launched, 0 when it
 * returned before the launch. */
int orbm_debug_last_refine_sim3_waits(void);

/* ------------------------------------------------------------------ pose-only optimisation
 * Optimizer::PoseOptimization(Frame *pFrame)   src/Optimizer.cc:264-476, the g2o graph it builds and the Levenberg loop g2o runs on
 * it (one VertexSE3Expmap, an EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose with a Huber kernel per keypoint that
 * holds a map point, 4 rounds x 10 iterations, inlier / outlier classification between rounds) in ONE launch per call, one
 * workgroup per problem.  The frame is passed flat, by keypoint index i < n (at most 8,192):
 *   kps_un[i]      mvKeysUn[i] (pt, octave)           uright[i]   mvuRight[i] (< 0: monocular edge; NULL: every edge monocular)
 *   has_mp[i]      mvpMapPoints[i] != NULL            mp_pos[i][3]  mvpMapPoints[i]->GetWorldPos()
 *   Tcw_in         mTcw (4 x 4 row-major floats)      Tcw_out     what SetPose receives (= Tcw_in with fewer than 3 map points)
 *   outlier[i]     mvbOutlier[i], written only where has_mp[i]
 *   *ngood         the return value, nInitialCorrespondences - nBad
 * Results are the same bits from run to run and whether a problem runs alone or in a batch. */
typedef struct orbm_pose_camera {
    float fx, fy, cx, cy, bf;           /* Frame::fx, fy, cx, cy, mbf */
    int32_t nlevels;                    /* mvInvLevelSigma2.size(), 1..32 */
    const float *inv_level_sigma2;      /* Frame::mvInvLevelSigma2 (host memory) */
} orbm_pose_camera;
/* Optional out-struct (test aid): what the rounds did, and the estimate in double before Converter::toCvMat. */
typedef struct orbm_pose_stats {
    int32_t rounds;                     /* rounds run: 4, 1 with fewer than 10 edges, 0 with fewer than 3 */
    int32_t iterations[4];              /* SparseOptimizer::optimize iterations (Levenberg solve() calls) per round */
    int32_t trials[4];                  /* damped-system solves (Levenberg trials) per round */
    int32_t ninitial;                   /* nInitialCorrespondences */
    double chi2;                        /* currentChi after the last iteration of the last round (0 if it had none) */
    double q[4];                        /* final estimate: rotation x y z w ... */
    double t[3];                        /* ... and translation */
} orbm_pose_stats;
/* Single call, host arrays. */
int orbm_pose_optimization(const orbx_keypoint *kps_un, const float *uright, int n, const uint8_t *has_mp, const float *mp_pos,
                           const orbm_pose_camera *cam, const float *Tcw_in, float *Tcw_out, uint8_t *outlier, int *ngood,
                           orbm_pose_stats *stats);
/* Single call on a resident frame: mvKeysUn and mvuRight are the frame handle's (orbm_frame_create / _from_extractor, in HBM), so
 * per call only has_mp[n] and mp_pos[n][3] travel, by keypoint index.  Same results as orbm_pose_optimization, bit for bit. */
int orbm_frame_pose_optimization(const orbm_frame *frame, const uint8_t *has_mp, const float *mp_pos, const orbm_pose_camera *cam,
                                 const float *Tcw_in, float *Tcw_out, uint8_t *outlier, int *ngood, orbm_pose_stats *stats);
/* B problems in one launch (the relocalisation candidates of Tracking::Relocalization): problem p owns keypoints
 * kp_off[p] .. kp_off[p + 1] - 1 of kps_un / uright / has_mp / mp_pos / outlier (kp_off[0] = 0), Tcw_in[p][16], Tcw_out[p][16],
 * ngood[p], stats[p] (or NULL); one camera.  is_device = 0: host arrays, synchronous.  is_device = 1: every array (kp_off
 * included) is in device memory and the call only enqueues the launch on `stream` (NULL: the null stream); a problem with more
 * than 8,192 keypoints then gets ngood[p] = ORBX_ERR_UNSUPPORTED, and one with a keypoint that has a map point and an octave
 * outside [0, nlevels) gets ngood[p] = ORBX_ERR_ARG (the host forms refuse both before the launch); such a problem writes no
 * other output, and the other problems of the batch are unaffected. */
int orbm_pose_optimization_batch(const orbx_keypoint *kps_un, const float *uright, const int32_t *kp_off, int batch, const uint8_t *has_mp,
                                 const float *mp_pos, const orbm_pose_camera *cam, const float *Tcw_in, float *Tcw_out, uint8_t *outlier,
                                 int32_t *ngood, orbm_pose_stats *stats, int is_device, void *stream);

/* ------------------------------------------------------------------ a frame tracked in one call
 * The two functions the tracking thread runs on every frame, each as ONE call: the projection search chained into the pose solve
 * on one stream -- prefix, window search, resolver, pose kernel -- with one staged upload and one host wait; the pose kernel forms
 * its edges on the device from the resolver's match_kp (no has_mp / mp_pos array is built on the host) and counts the matches
 * that survive in its epilogue.  Results are, bit for bit, those of the search call followed by orbm_frame_pose_optimization
 * over the gathered matches.  When the search has to be repeated (a window list that outgrew its region, a resolver that did not
 * reach its fixed point, too few matches) the pose kernel leaves without solving and the host repeats the chain: more waits, same
 * results.  The frame's mvKeysUn / mvuRight are the handle's.  At most 8,192 keypoints (ORBX_ERR_UNSUPPORTED); a keypoint octave
 * outside [0, nlevels) of the view or of the pose camera is ORBX_ERR_ARG; both before anything is launched. */
typedef struct orbm_track_result {
    int32_t tracked;                    /* 0: fewer than min_matches after both searches, no pose solve (Tracking.cc:1251-1252) */
    int32_t search_used;                /* 1: the search with th, 2: the one with 2 * th (:1245-1249) */
    int32_t nsearch;                    /* what that search returned */
    int32_t ngood;                      /* PoseOptimization's return value */
    int32_t nmatches;                   /* slots that hold a point and are not outliers (:1271; mnMatchesInliers with mbOnlyTracking, :1314) */
    int32_t nmatches_map;               /* ... of them, those whose point has Observations() > 0 (nmatchesMap :1274; mnMatchesInliers :1311) */
} orbm_track_result;
/* Tracking::TrackWithMotionModel   src/Tracking.cc:1232-1284 (behind UpdateLastFrame): SearchByProjection(Cur, Last, th, mono) with
 * every slot free (mvpMapPoints was filled with NULL, :1234), again from scratch with 2 * th if it returns fewer than min_matches
 * (20 in the reference, :1245-1249); if still fewer: result->tracked = 0, Tcw_out = Tcw, outlier untouched (:1251-1252).  Else
 * PoseOptimization from Tcw over the matches (keypoint j holds the point last->pos[match_kp[j]] iff match_kp[j] >= 0) and the
 * counts of the discard loop (:1257-1276).  Tcw = mVelocity * mLastFrame.mTcw: the pose the search projects with AND the
 * solve's start (:1232).  last, th, mono, th_high, check_orientation as for orbm_search_by_projection_last.  match_kp[n] /
 * match_q[last->n] are returned as the accepted search left them (the discard does not edit them: -1 never matched, -2 cleared
 * by the rotation check, an outlier keeps its index); outlier[n] is written only where match_kp[j] >= 0.  stats may be NULL. */
int orbm_track_with_motion_model(const orbm_frame *cur, const orbm_view *view, const orbm_pose_camera *cam, const float *Tcw, const float *Tlw,
                                 const orbm_points *last, float th, int mono, int th_high, int check_orientation, int min_matches,
                                 int32_t *match_kp, int32_t *match_q, uint8_t *outlier, float *Tcw_out, orbm_track_result *result,
                                 orbm_pose_stats *stats);
/* Tracking::TrackLocalMap   src/Tracking.cc:1294-1320 (behind UpdateLocalMap): SearchLocalPoints as
 * orbm_search_by_projection_points (points, th, viewing_cos_limit, th_high, nnratio as there), then PoseOptimization from Tcw over the
 * UNION of the new matches and the slots the frame holds already, given by keypoint index: base_has[n] (mvpMapPoints[j] != NULL),
 * base_pos[n][3] (its GetWorldPos()), base_takes[n] (its Observations() > 0; NULL: all).  occupied[j] = base_has[j] && base_takes[j]
 * is derived here (ORBmatcher.cc:87-89); a new match overrides the base entry of its slot (the reference overwrites
 * mvpMapPoints[idx]).  base_has may be NULL (the frame holds nothing).  Then the counts of :1301-1320: result->nmatches_map =
 * mnMatchesInliers, result->nmatches = the same with mbOnlyTracking.  outlier[n] is written where the union holds a point;
 * dropping stereo outliers from mvpMapPoints (:1316-1317) stays the caller's.  result->tracked = 1, search_used = 1 always.
 * projected_out (optional) as for orbm_search_by_projection_points. */
int orbm_track_local_map(const orbm_frame *cur, const orbm_view *view, const orbm_pose_camera *cam, const float *Tcw, const orbm_points *points,
                         const uint8_t *base_has, const float *base_pos, const uint8_t *base_takes, float th, float viewing_cos_limit,
                         int th_high, float nnratio, int32_t *match_kp, int32_t *match_q, orbm_projected_point *projected_out,
                         uint8_t *outlier, float *Tcw_out, orbm_track_result *result, orbm_pose_stats *stats);
/* Host waits (stream synchronisations) of the last orbm_track_* call of this process: 1 on the common path. */
int orbm_debug_last_track_waits(void);

/* ------------------------------------------------------------------ bundle adjustment
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:837-1162) and Optimizer::BundleAdjustment (:74-262) on the graph the caller
 * has flattened: g2o's Levenberg loop (optimization_algorithm_levenberg.cpp:63-241) runs on the host and drives
 * device passes -- errors + robust chi2, build, Schur complement, a dense LLT of the reduced system, back-substitution + update --
 * with one host wait per trial and one per round.
 *   poses      [nfree + nfixed][16]: GetPose() of the local keyframes (lLocalKeyFrames order), then of the fixed ones
 *   fixed      [nfree] or NULL: 1 = this local keyframe is a fixed vertex (mnId == 0, :913)
 *   points     [npoints][3]: GetWorldPos()
 *   edges      grouped by point, points ascending, within a point in the observations map's order: e_point, e_cam (an index
 *              into poses), e_obs = (u, v, ur) with ur < 0 for a monocular edge, e_inv_sigma2 = mvInvLevelSigma2[octave],
 *              e_cam_k = fx fy cx cy bf of the observing keyframe.  A keyframe observes a point at most once.
 * Limits (ORBX_ERR_UNSUPPORTED before any device work, nothing written): nfree <= 64, nfixed <= 1,024, npoints <= 65,536,
 * nedges <= 524,288.  ORBX_ERR_ARG: a NULL array, a negative size, an index out of range, edges not grouped by ascending point, a
 * keyframe that observes a point twice, an option outside its range.  nfree = 0 or nedges = 0: the input is returned, no launch. */
typedef struct orbm_ba_graph {
    int32_t nfree, nfixed, npoints, nedges;
    const float *poses;
    const uint8_t *fixed;
    const float *points;
    const int32_t *e_point, *e_cam;
    const float *e_obs, *e_inv_sigma2, *e_cam_k;
} orbm_ba_graph;
/* nrounds 1 or 2, iterations[r] 0 .. 64 = optimize(n) of round r.  Round 0 carries Huber kernels iff robust_round0 (huber_mono /
 * huber_stereo = delta, the double of the reference's float); round 1 never does.  classify: after round 0 an edge whose stored
 * chi2 is > chi2_mono / chi2_stereo or whose point is not in front of its camera goes to level 1 (:1043-1087), and after the last
 * round the same test fills result->erase (:1091-1127).  The two uses: */
typedef struct orbm_ba_options {
    int32_t nrounds, iterations[2], robust_round0, classify;
    int32_t reserved;
    double huber_mono, huber_stereo, chi2_mono, chi2_stereo;
} orbm_ba_options;
/* LocalBundleAdjustment: optimize(5), the level pass, optimize(10); (float)sqrt(5.991), (float)sqrt(7.815) */
#define ORBM_BA_OPTIONS_LOCAL {2, {5, 10}, 1, 1, 0, 2.4476518630981445, 2.7955322265625, 5.991, 7.815}
/* BundleAdjustment(nIterations, bRobust): one round, no level pass; (float)sqrt(5.99) -- not 5.991 -- and (float)sqrt(7.815) */
#define ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust) {1, {(nIterations), 0}, (bRobust) ? 1 : 0, 0, 0, 2.4474475383758545, 2.7955322265625, 5.99, 7.815}
typedef struct orbm_ba_result {
    float *poses;                       /* [nfree][16]: what SetPose receives (the fixed keyframe too: its pose through toSE3Quat / toCvMat) */
    float *points;                      /* [npoints][3] */
    uint8_t *erase;                     /* [nedges]: the edge is in vToErase; written iff classify (may be NULL otherwise) */
    uint8_t *not_included;              /* [npoints] or NULL: the point has no edge (BundleAdjustment :200-208) */
    int32_t stopped;                    /* 0 ran to the end; 1 the stop flag was set before the first optimize (nothing changed);
                                           2 it was seen later (behind the first round: bDoMore = false, no level pass and no second round;
                                           the final pass still ran) */
} orbm_ba_result;
typedef struct orbm_ba_trial {
    double tempChi, currentChi, rho, lambda, scale;     /* lambda: after the trial's update of it */
    int32_t round, qmax, accepted, ok2;
} orbm_ba_trial;
/* Optional out-struct (test aid).  trial_log / poses / points / chi2 / level are the caller's arrays (or NULL). */
typedef struct orbm_ba_stats {
    int32_t rounds;                     /* rounds that ran optimize() */
    int32_t iterations[2], trials[2];
    int32_t nresults;
    int32_t results[128];               /* SolverResult of every iteration: 1 OK, 2 Terminate */
    int32_t trial_capacity, ntrials, trial_overflow;
    orbm_ba_trial *trial_log;           /* [trial_capacity] */
    double *poses;                      /* [nfree][7]: the final estimates, q (x y z w) and t */
    double *points;                     /* [npoints][3] */
    double *chi2;                       /* [nedges]: chi2() of the edge's stored error */
    uint8_t *level;                     /* [nedges] */
} orbm_ba_stats;
/* stop_flag (or NULL) = pbStopFlag: read where g2o reads it (before each iteration, in the trial loop's condition) and where
 * LocalBundleAdjustment does (:1039-1041, :1047-1049). */
int orbm_bundle_adjustment(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag, orbm_ba_result *out,
                           orbm_ba_stats *stats);
/* Host only, no device: the index lists the call would use.  Any output may be NULL.
 *   pose_class[nfree + nfixed]   0 free and connected, 1 fixed, 2 free without an edge (not a vertex of the system)
 *   point_class[npoints]         0 connected, 1 without an edge
 *   pose_edge_start[nfree + 1], pose_edges[]   a free keyframe's edges, ascending (a fixed local keyframe: none)
 *   block_start[nfree (nfree + 1) / 2 + 1], block_entries[][3]   block (i1 <= i2) has index i1 nfree - i1 (i1 - 1) / 2 + i2 - i1;
 *                                its entries (point, edge of i1, edge of i2), points ascending
 *   counts[2]                    entries of pose_edges and of block_entries (call once with NULL lists to size them) */
int orbm_ba_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                 int32_t *block_start, int32_t *block_entries, int32_t *counts);
/* Host waits of the last orbm_bundle_adjustment or orbm_global_bundle_adjustment of this process: trials + rounds (the stop flag
 * seen behind the first round saves that round's wait); 0 when nothing was launched. */
int orbm_debug_last_ba_waits(void);
/* The same call for a map of up to 512 keyframes (the global BA behind a loop closure, LoopClosing::RunGlobalBundleAdjustment;
 * DESIGN.md 25): signatures, structs, options (either ORBM_BA_OPTIONS_* form), stop flag, waits and every documented deviation as
 * orbm_bundle_adjustment / orbm_ba_plan.  What differs: nfree <= 512 (nfixed, npoints, nedges as above), and block_entries may hold at
 * most 2^25 = 33,554,432 entries (ORBX_ERR_UNSUPPORTED before any device work, nothing written; no graph the other entry admits
 * exceeds it).  The reduced system, up to 3,072 wide, is ALWAYS solved by orbm_llt_solve_dev, at every size: a graph both entries
 * admit gives the same bytes through either.  The leased workspace grows to about 80 MB at 512 keyframes and stays leased to the
 * process like every arena. */
int orbm_global_bundle_adjustment(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag, orbm_ba_result *out,
                                  orbm_ba_stats *stats);
int orbm_global_ba_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                        int32_t *block_start, int32_t *block_entries, int32_t *counts);
/* The same call for the map of a long session, up to 4,096 keyframes: structs, options (either ORBM_BA_OPTIONS_* form),
 * stop flag, waits (trials + rounds) and every documented deviation as orbm_global_bundle_adjustment.  What differs: the reduced
 * system is assembled into the live tiles of its TILE ENVELOPE and solved by orbm_llt_env_solve_dev (below), at every size; the
 * n x n square is never allocated.  Limits (ORBX_ERR_UNSUPPORTED before any device work, nothing written; the call refuses what
 * orbm_global_ba_env_plan refuses): nfree <= 4,096, nfixed <= 1,024, npoints <= 1,048,576, nedges <= 4,194,304, block_entries <= 2^26 =
 * 67,108,864, and at most 8,192 live tiles in round 0 (checked behind every ORBX_ERR_ARG of the graph, the options and the result).
 * Rows are the caller's order of the free keyframes, and that order decides the envelope: block (i1 <= i2) of two keyframes that share a
 * map point covers rows 6 r2 .. 6 r2 + 5 from column 6 r1 (r = the keyframe's rank among the vertices of the round), and row tile R
 * (T = orbm_llt_tile() rows) starts at the smallest column tile a block reaching it has.  LIST THEM BY ASCENDING mnId: covisibility is
 * local in time, so the blocks then form a band, and the points re-observed at a loop widen only the rows of the later keyframes; a
 * shuffled list gives a wide envelope, more work, and past the tile cap a refusal.  Every entry of the system has the value
 * orbm_global_bundle_adjustment gives it (the same operations in the same order; an empty block between two vertices is +0.0 in
 * both), and the solver skips only products with exact zeros: a graph both entries admit gives the same numbers through either.
 * THE SECOND ROUND (nrounds = 2): keyframes that left the system compact the rows, so round 1 has an envelope of its own.  The
 * read-back between the rounds brings the rows, the envelope is planned again on the host and its image uploaded: no further wait.
 * A two-round call reserves min(2 live + nt, the full triangle, 8,192) tiles (live, nt: round 0's live tiles and row tiles), which
 * holds every second round but for the solver's cap: if round 1's envelope has more than 8,192 live tiles the call returns
 * ORBX_ERR_UNSUPPORTED behind round 0, with the result arrays untouched (the statistics are reset).  The leased workspace holds two copies of the live tiles (up
 * to 2 x 256 MiB) and stays leased to the process like every arena.
 *
 * orbm_global_ba_env_plan: host only, no device; pose_class, point_class, pose_edge_start, pose_edges as orbm_ba_plan, then the COMPACT
 * block list -- the non-empty upper blocks alone, sorted by (i1, i2) -- and round 0's envelope.  Any output may be NULL.
 *   blk_i1[counts[2]], blk_i2[counts[2]]   the listed blocks; the diagonal block of every free, connected keyframe is among them
 *   blk_start[counts[2] + 1], block_entries[counts[1]][3]   a block's entries (point, edge of i1, edge of i2), points ascending: the
 *                            concatenation is orbm_global_ba_plan's block_entries with the empty blocks left out
 *   first[counts[3]]         round 0's envelope: first live column tile of every row tile (orbm_llt_env_plan takes it from there)
 *   counts[6]                entries of pose_edges, of block_entries, listed blocks, row tiles, live tiles, kernel launches of one solve
 * so a caller can see what an ordering costs before it calls. */
int orbm_global_bundle_adjustment_env(const orbm_ba_graph *g, const orbm_ba_options *opt, const volatile uint8_t *stop_flag,
                                      orbm_ba_result *out, orbm_ba_stats *stats);
int orbm_global_ba_env_plan(const orbm_ba_graph *g, int32_t *pose_class, int32_t *point_class, int32_t *pose_edge_start, int32_t *pose_edges,
                            int32_t *blk_i1, int32_t *blk_i2, int32_t *blk_start, int32_t *block_entries, int32_t *first, int32_t *counts);

/* ------------------------------------------------------------------ tiled dense Cholesky solve
 * S x = b for a symmetric positive definite S of 1 <= n <= 3,072 rows, over many workgroups, in T x T tiles (T = orbm_llt_tile()).
 * Everything is DEVICE memory; the call is asynchronous on `stream`, waits for nothing on the host and allocates nothing.
 *   S_dev   [n][n] column-major: entry (row i, column j) is S[j * n + i].  Only i >= j is read as input.  On return the lower
 *           triangle holds L with S = L L^T; the strict upper triangle is the call's scratch (written before read, contents
 *           unspecified afterwards)
 *   b_dev   [n], read only; must not overlap x_dev
 *   x_dev   [n]: the solution (scratch of the call until then)
 *   ok_dev  one word: 1, or 0 when a pivot was not > 0 (<= 0 or NaN); then x = 0.0 everywhere and L is unspecified.  Both are
 *           written on every path; the host never reads the word
 * The arithmetic, operation by operation (plain double multiplies and adds, no fused multiply-add, no matrix instruction, no
 * floating-point atomic), which makes the result independent of T and equal to the one-workgroup solve of orbm_bundle_adjustment:
 *   L[i][j] = (a[i][j] - dot) / L[j][j], pivot L[j][j] = sqrt(a[j][j] - dot); column 0 has no dot
 *   dot = L[i][0] L[j][0] (not 0.0 + it), then dot = dot + L[i][k] L[j][k] for k = 1 .. j - 1 in ascending k
 *   y_i = b_i, y_i -= L[i][j] y_j for j = 0 .. i - 1 ascending, then y_i / L[i][i]
 *   x_i = y_i, x_i -= L[j][i] x_j for j = n - 1 .. i + 1 descending, then x_i / L[i][i]
 * n outside 1 .. 3,072 or a NULL pointer: ORBX_ERR_ARG before any device work.  4 ceil(n / T) - 1 launches. */
int orbm_llt_tile(void);
int orbm_llt_solve_dev(int n, double *S_dev, const double *b_dev, double *x_dev, int32_t *ok_dev, void *stream);
/* Kernel launches of the last orbm_llt_solve_dev or orbm_llt_env_solve_dev of this process. */
int orbm_debug_last_llt_launches(void);

/* ------------------------------------------------------------------ tiled Cholesky solve over a tile envelope
 * The same solve for a sparse S of 1 <= n <= 28,672 rows whose non-zeros lie inside a TILE ENVELOPE.  With
 * T = orbm_llt_tile() and nt = ceil(n / T), first[R] (0 <= first[R] <= R, host memory, need not be monotone) is the first live column
 * tile of row tile R: the tiles (R, C), first[R] <= C <= R, are LIVE, every other tile is structurally zero and is neither stored
 * nor touched.  Cholesky fill stays inside such an envelope.  At most 8,192 live tiles (2 x 256 MiB of tiles): every envelope up to
 * nt = 127, the full one included, fits.
 *   A_dev    the live tiles, packed: tile (R, C) is tile number off[R] + C - first[R], off[R] = sum over r < R of r - first[r] + 1,
 *            each tile T x T doubles COLUMN-major (entry (R T + i, C T + j) at j * T + i).  EVERY entry of a live tile with a row
 *            below n is input, the zeros too; of a diagonal tile only i >= j is read.  On return the tiles hold L.  Rows at or
 *            beyond n of the last row tile, and the strict upper part of a diagonal tile, are never read or written
 *   W_dev    as many doubles as A_dev: the running dots, the call's scratch (written before read, unspecified afterwards).  The
 *            dense solver keeps them in the mirrored triangle and in x; a packed triangle has no mirror, so the caller lends the
 *            room.  The diagonal's dots are on W's diagonal (no further array)
 *   b_dev, x_dev, ok_dev   as orbm_llt_solve_dev
 *   plan_dev int32, device: first[nt], off[nt + 1], row_start[nt + 1], rows[row_start[nt]] of orbm_llt_env_plan, one after the other.
 *            The caller uploads it (once per call, or once for many calls with the same envelope); the solver reads `first` on the
 *            host for its grids and never waits
 * The arithmetic is orbm_llt_solve_dev's, entry by entry, restricted to live tiles: the dot of an entry of tile (R, C) STARTS as its
 * first product of panel max(first[R], first[C]) and adds the later panels' products in ascending k; a tile whose row and column
 * start at itself has no dot; y_i takes the panels first[R] .. R - 1 ascending, x_i the rows R' with first[R'] <= R descending.  On a
 * matrix that is zero outside the envelope, L's live tiles and x equal the dense solver's as numbers (the products it skips are
 * +-0.0, so the sign of a zero may differ and nothing else); ok is the same.  Failure as there: ok = 0, x = 0.0 everywhere.
 * Launches: 1 + 2 nt + per panel K < nt - 1 one (two when a row tile has first[R] <= K < R), at most 4 nt - 1; never an empty grid.
 * ORBX_ERR_ARG: n outside 1 .. 28,672, a first[R] outside 0 .. R, a NULL pointer; ORBX_ERR_UNSUPPORTED: more than 8,192 live tiles;
 * both before any device work, nothing written.
 *
 * orbm_llt_env_plan: host only, no device; what the solver will do for n and first[].  Any output may be NULL.
 *   off[nt + 1]           tile number of (R, first[R]); off[nt] = the live tiles
 *   row_start[nt + 1], rows[]     panel K's row tiles: R > K with first[R] <= K, ascending (the tiles that solve against diagonal
 *                         tile K, subtract y_K in the forward pass and give x_K its terms in the backward pass)
 *   trail_start[nt + 1], trail[][2]   panel K's trailing tiles (R, C), K < C <= R, first[R] <= K and first[C] <= K, by R then C: the
 *                         pairs of panel K's row tiles
 *   counts[4]             live tiles, entries of rows, trailing tiles, launches (call once with NULL lists to size them) */
int orbm_llt_env_plan(int n, const int32_t *first, int32_t *off, int32_t *row_start, int32_t *rows, int32_t *trail_start, int32_t *trail,
                      int32_t *counts);
int orbm_llt_env_solve_dev(int n, const int32_t *first, const int32_t *plan_dev, double *A_dev, double *W_dev, const double *b_dev,
                           double *x_dev, int32_t *ok_dev, void *stream);

/* ------------------------------------------------------------------ essential graph
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1165-1428): the Sim3 pose graph LoopClosing::CorrectLoop
 * optimises between SearchAndFuse and the global BA, on the graph the caller has flattened.  The caller only walks pointers: vScw,
 * the measurements Sji, the 20 Levenberg iterations, the SE3 recovery and the map-point correction are the call's.  g2o's Levenberg
 * loop runs on the host and drives device passes -- errors + chi2, g2o's NUMERIC Jacobians of every edge, the 7-wide blocks into a
 * dense system, orbm_llt_solve_dev (at every size), the update -- with one host wait per trial and one at the end.
 *   poses              [nvert][16]: GetPose() of every non-bad keyframe, in vpKFs order
 *   corrected          [nvert]: row of corrected_sim3 [ncorr][8] (q xyzw, t, s: the CorrectedSim3 entry), or -1
 *   noncorrected       [nvert]: the same into noncorrected_sim3 [nnc][8]
 *   fixed              [nvert]: 1 = pLoopKF
 *   edges              in the reference's creation order (:1236-1367): e_v0 = nIDi (vertex 0), e_v1 = nIDj (vertex 1), e_kind 0 = an
 *                      edge of the LoopConnections loop (Sji = vScw[j] vScw[i]^-1), 1 = a spanning-tree, old-loop or covisibility edge
 *                      (each side takes its NonCorrectedSim3 where it has one, else vScw)
 *   points, p_ref      [npoints][3] GetWorldPos(), and the vertex index of the keyframe :1404-1413 choose
 * Limits (ORBX_ERR_UNSUPPORTED before any device work, nothing written): nact <= 438 (the free vertices that have an edge: the system
 * is 7 nact wide and orbm_llt_solve_dev takes 3,072), nvert <= 1,024, nedges <= 32,768, npoints <= 1,048,576.  ORBX_ERR_ARG: a NULL
 * array, a negative size, an index out of range, e_v0 == e_v1, an edge between two fixed vertices, a non-finite input value,
 * iterations outside 0 .. 64, lambda_init not positive and finite.  nedges = 0, nact = 0 or iterations = 0: no solve; the
 * conversions and the point correction still run on the unchanged estimates. */
typedef struct orbm_eg_graph {
    int32_t nvert, ncorr, nnc, nedges, npoints, fix_scale;
    const float *poses;
    const int32_t *corrected;
    const double *corrected_sim3;
    const int32_t *noncorrected;
    const double *noncorrected_sim3;
    const uint8_t *fixed;
    const int32_t *e_v0, *e_v1;
    const uint8_t *e_kind;
    const float *points;
    const int32_t *p_ref;
} orbm_eg_graph;
typedef struct orbm_eg_options {
    int32_t iterations;                 /* optimize(n), 0 .. 64 */
    int32_t reserved;
    double lambda_init;                 /* setUserLambdaInit: > 0 */
} orbm_eg_options;
#define ORBM_EG_ITERATIONS 20
#define ORBM_EG_OPTIONS_DEFAULT {ORBM_EG_ITERATIONS, 0, 1e-16}
typedef struct orbm_eg_result {
    float *poses;                       /* [nvert][16]: [R | t / s] as :1383-1393 form it, of every vertex (the fixed and the edgeless too) */
    float *points;                      /* [npoints][3]: correctedSwr.map(Srw.map(P)) */
} orbm_eg_result;
/* Optional out-struct (test aid).  trial_log / estimates / chi2 are the caller's arrays (or NULL).  A trial's `round` is 0. */
typedef struct orbm_eg_stats {
    int32_t iterations, trials;
    int32_t nresults;
    int32_t results[64];                /* SolverResult of every iteration: 1 OK, 2 Terminate */
    int32_t trial_capacity, ntrials, trial_overflow;
    orbm_ba_trial *trial_log;           /* [trial_capacity] */
    double *estimates;                  /* [nvert][8]: the final estimates, q (x y z w), t, s */
    double *chi2;                       /* [nedges]: chi2() of the edge's stored error */
} orbm_eg_stats;
int orbm_essential_graph(const orbm_eg_graph *g, const orbm_eg_options *opt, orbm_eg_result *out, orbm_eg_stats *stats);
/* Host only, no device: the index lists the call would use.  Any output may be NULL.
 *   vertex_class[nvert]      0 free with an edge (a vertex of the system), 1 fixed, 2 free without an edge
 *   row[nvert]               block row of a class-0 vertex in the system (ascending in vertex order), else -1
 *   vert_edge_start[nvert + 1], vert_edges[]   a class-0 vertex's edges in edge order, as 2 edge + side (side: the vertex is vertex 0 / 1)
 *   pair_start[npairs + 1], pair_v[npairs][2], pair_edges[]   the pairs of class-0 vertices an edge joins, ascending by (smaller row,
 *                            larger row); pair_v = (vertex of the smaller row, of the larger); its edges in edge order as 2 edge + o,
 *                            o = 1 when the edge's vertex 0 has the larger row
 *   counts[3]                entries of vert_edges, pairs, entries of pair_edges (call once with NULL lists to size them) */
int orbm_eg_plan(const orbm_eg_graph *g, int32_t *vertex_class, int32_t *row, int32_t *vert_edge_start, int32_t *vert_edges,
                 int32_t *pair_start, int32_t *pair_v, int32_t *pair_edges, int32_t *counts);
/* Host waits of the last orbm_essential_graph or orbm_essential_graph_env of this process: trials + 1; 0 when nothing was launched. */
int orbm_debug_last_eg_waits(void);
/* The same call for the essential graph of a long session: structs, options, statistics, waits and every documented
 * deviation as orbm_essential_graph.  What differs: the system is assembled into the live tiles of a TILE ENVELOPE and solved by
 * orbm_llt_env_solve_dev, so the limits are nact <= 4,096 (a system 28,672 wide), nvert <= 8,192, nedges <= 131,072, npoints <=
 * 1,048,576 and at most 8,192 live tiles (ORBX_ERR_UNSUPPORTED before any device work, nothing written; the tile cap is checked
 * behind every ORBX_ERR_ARG of the graph, the options and the result, and also when iterations = 0 or nothing would be solved: the call
 * refuses what orbm_eg_env_plan refuses).  Rows are the caller's
 * vertex order, and that order decides the envelope: row tile R of the system (7 rows per class-0 vertex, T = orbm_llt_tile() rows
 * per tile) starts at the smallest column tile any of its vertices' pairs reaches.  LIST THE KEYFRAMES BY ASCENDING mnId: spanning-
 * tree and covisibility edges then join neighbours in the list and form a band a few tiles wide, and a loop edge widens only the
 * rows of its later keyframe; a shuffled list gives a wide envelope, more work, and past the tile cap a refusal.  Every entry of the
 * system has the value orbm_essential_graph gives it (same sums in the same order), and the solver skips only products with exact
 * zeros: a graph both entries admit gives the same numbers through either (the sign of a zero inside the solve aside).  The leased
 * workspace holds two copies of the live tiles (up to 2 x 256 MiB) and stays leased to the process like every arena.
 *
 * orbm_eg_env_plan: host only, no device; what orbm_eg_plan returns under the limits above, plus
 *   first[counts[3]]         the envelope: first live column tile of every row tile (orbm_llt_env_plan takes it from there)
 *   counts[6]                the three of orbm_eg_plan, then row tiles, live tiles, kernel launches of one solve
 * so a caller can see what an ordering costs before it calls.  Refuses what the call refuses. */
int orbm_essential_graph_env(const orbm_eg_graph *g, const orbm_eg_options *opt, orbm_eg_result *out, orbm_eg_stats *stats);
int orbm_eg_env_plan(const orbm_eg_graph *g, int32_t *vertex_class, int32_t *row, int32_t *vert_edge_start, int32_t *vert_edges,
                     int32_t *pair_start, int32_t *pair_v, int32_t *pair_edges, int32_t *first, int32_t *counts);

/* KeyFrameDatabase on the device (src/KeyFrameDatabase.cc:40-309, src/LoopClosing.cc:120-141): the BowVectors of the
 * added keyframes live in HBM, one row of (word id, value) per keyframe under a SLOT number.  Slots are handed out in ascending
 * order of add and are not reused before clear, so slot order is the order of the reference's inverted lists.  nwords = the
 * vocabulary's size.  A row or a query holds 0 .. 8,192 words, ids strictly ascending inside [0, nwords) (a BowVector as
 * std::map iterates it), values as Frame::ComputeBoW leaves them.  ORBX_ERR_ARG, with the reason in orbx_last_error(), before
 * anything is launched or written: ids not strictly ascending or outside [0, nwords), n or nq negative or above 8,192, a dead or
 * out-of-range slot (erase, score), a second erase of a slot, a NULL output.  Arguments are checked first, then the device
 * (ORBX_ERR_NO_DEVICE); create, clear, size and destroy need none, nor does a query or score call that launches nothing.  A database may be used from several threads (one call at a
 * time runs; the reference holds a mutex too).
 *   add      uploads the row (the store grows by itself and keeps what is resident); *slot = its slot.  One host wait.
 *   erase    marks the slot dead; the row stays where it is until clear (dead rows are never compacted in between).
 *   clear    forgets every slot (the next add gets slot 0) and keeps the capacity.
 *   size     *live = keyframes in the database, *slots = slots handed out since the last clear (either may be NULL).
 *   query    fills common[slots], first[slots], score[slots] for EVERY slot:
 *              dead slot   common -1, first -1, score +0.0f
 *              live slot   common = words it shares with the query, first = index INTO THE QUERY of the first shared word (-1:
 *                          none), score = (float)DBoW2::L1Scoring::score(query, row): the double sum of |vi - wi| - |vi| - |wi|
 *                          over the shared words in ascending word id, then -sum / 2.0 -- bit for bit (-0.0f when nothing is shared)
 *            One staged upload (the query), one launch, one host wait.  No live keyframe or nq = 0: the rows are filled as above
 *            (common 0 / -1) and nothing is launched.  Scores are computed for every sharing keyframe, also those the caller's 0.8
 *            cut on common drops.
 *   score    the same score for a list of n <= 8,192 live slots (a slot may repeat): LoopClosing::DetectLoop's minScore loop.  One
 *            upload, one launch, one wait; n = 0: nothing is launched. */
typedef struct orbm_kfdb orbm_kfdb;
int orbm_kfdb_create(int nwords, orbm_kfdb **out);
int orbm_kfdb_destroy(orbm_kfdb *db);
int orbm_kfdb_add(orbm_kfdb *db, const int32_t *words, const double *values, int n, int32_t *slot);
int orbm_kfdb_erase(orbm_kfdb *db, int slot);
int orbm_kfdb_clear(orbm_kfdb *db);
int orbm_kfdb_size(const orbm_kfdb *db, int *live, int *slots);
int orbm_kfdb_query(orbm_kfdb *db, const int32_t *qwords, const double *qvalues, int nq, int32_t *common, int32_t *first, float *score);
int orbm_kfdb_score(orbm_kfdb *db, const int32_t *qwords, const double *qvalues, int nq, const int32_t *slots, int n, float *score);
/* Host waits of the last orbm_kfdb_query / orbm_kfdb_score of this process: 1 when it launched, 0 when nothing was launched. */
int orbm_debug_last_kfdb_waits(void);
/* How often the store replaced a device pool by a larger one since create (-1: NULL database). */
int orbm_debug_kfdb_reallocs(const orbm_kfdb *db);
/* Test aid: at most `blocks` workgroups per orbm_kfdb_query / orbm_kfdb_score launch instead of 2,048 (0: the default again), so that
 * a few keyframes already make every wave stride over several slots.  Same results.  Process-wide; returns the previous setting. */
int orbm_debug_kfdb_max_blocks(int blocks);

/* Test aid: on != 0 makes the whole-loop projection searches use the one-wave sequential resolver (k_resolve) instead of the
 * parallel fixed-point resolver (k_resolve_par), which otherwise only takes over when the latter does not converge.  Both
 * give the reference loop's result.  Process-wide; returns the previous setting. */
int orbm_debug_force_sequential_resolver(int on);
/* Iterations the parallel resolver needed in the last whole-loop projection search of this process (-1: it gave up after
 * its iteration limit and the sequential resolver produced the result). */
int orbm_debug_last_resolver_iterations(void);
/* Host waits (stream synchronisations) of the last whole-loop search of this process that launched anything (orbm_search_projection,
 * orbm_search_for_initialization, orbm_search_by_bow, the orbm_search_by_projection_* forms, the orbm_track_* calls and their
 * frame forms): 1 on the common path; one more for every repeated attempt (a window list outgrew its region, the parallel resolver
 * did not settle) and for sizing the exact lists. */
int orbm_debug_last_search_waits(void);
/* Test aid: sets what the pooled scratch memory of the orbm_* calls holds before the next call ("What a call may assume
 * about its workspace").  Every workspace on the pool's free list -- one that a running call has leased is skipped and not counted --
 * gets its device arena and its entries buffer filled with the 32-bit `word` (on its own stream, waited for) and its pinned arena
 * likewise from the host.  as_next_generation != 0: `word` is ignored and each workspace is filled with the generation number its
 * NEXT call will use (the value a raised flag of that call has).  The pooled blocks of destroyed frames, which the next
 * orbm_frame_create takes as they are, are filled too: with `word`, or with the first free workspace's next generation (1 when
 * there is none).  *nworkspaces / *nframe_blocks = how many were filled.  Changes no call and sets nothing a kernel reads as a
 * switch; results never depend on it.  Needs a device. */
int orbm_debug_fill_workspaces(uint32_t word, int as_next_generation, int *nworkspaces, int *nframe_blocks);

/* Which kernel the all-pairs matchers (orbm_match_batch_dev, orbm_match_bruteforce) launch.  Both produce the same
 * integers.  ORBM_ALLPAIRS_AUTO (default): a matrix-core kernel (FP4 MFMA computes the selection keys, 4x
 * faster at 2000 x 2000; train tiles expanded once per workgroup and shared through LDS) for sets up to 32768 rows, the
 * XOR + popcount kernel above that; ORBM_ALLPAIRS_POPCOUNT: always the wavefront popcount + LDS-reduction kernel
 * BASELINE.json's north_star describes; ORBM_ALLPAIRS_MFMA: the matrix-core kernel that splits the train tiles over a
 * workgroup's waves (a little faster alone, more vector instructions).  Process-wide; returns the previous setting, or a
 * negative status for an unknown value. */
enum { ORBM_ALLPAIRS_AUTO = 0, ORBM_ALLPAIRS_POPCOUNT = 1, ORBM_ALLPAIRS_MFMA = 2 };
int orbm_set_allpairs_kernel(int kind);

/* HIP-event timing of the all-pairs kernel launched through orbm_match_batch_dev. */
int orbm_profile_enable(int on);
int orbm_profile_read(double *total_ms, int64_t *launches);
/* (orbm_profile_enable: bit 0 = the all-pairs matcher, bit 1 = orbm_bow_transform_batch_dev -- that kernel's own start and end events) */
int orbm_profile_read_bow(double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* ORBSLAM_HIP_H */
