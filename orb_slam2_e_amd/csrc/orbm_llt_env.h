// orbm_llt_env.h -- the plan image of a tile envelope (include/orbslam_hip.h, orbm_llt_env_solve_dev), written down once:
// the words first[nt] | off[nt + 1] | row_start[nt + 1] | rows[nrows] that the solver and the assembly kernels read on the device, and
// the host's way from a system's blocks to that image.  Internal: orbm_llt.hip, orbm_essential_graph.hip, orbm_ba.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/orbslam_hip.h"

// The four lists of an image of nt row tiles.  Live tile (R, C), first[R] <= C <= R, is packed tile number tile_index(R, C); panel K's
// row tiles (R > K with first[R] <= K) are rows[row_start[K]] .. rows[row_start[K + 1] - 1].
template <class I> struct LltEnvImage {
    I *first, *off, *row_start, *rows;
    LltEnvImage() = default;
    __host__ __device__ LltEnvImage(I *plan, int nt) : first(plan), off(plan + nt), row_start(off + nt + 1), rows(row_start + nt + 1) {}
    __host__ __device__ int tile_index(int R, int C) const { return off[R] + C - first[R]; }
    __host__ __device__ int col_of(int R, int t) const { return t - off[R] + first[R]; }       // C with tile_index(R, C) = t
    static size_t words(size_t nt, size_t nrows) { return 3 * nt + 2 + nrows; }
};
using LltEnvView = LltEnvImage<const int>;

// What a caller of orbm_llt_env_solve_dev plans on the host: first[] for the entry, the image for the device, the counts.
struct LltEnvPlan {
    int n = 0, nt = 0, live = 0, launches = 0;
    std::vector<int32_t> first, image;
};

// an envelope of n rows that nothing reaches yet: first[R] = R (n = 0: no row tile)
inline void llt_env_start(LltEnvPlan &E, int n)
{
    const int T = orbm_llt_tile();
    E = LltEnvPlan();
    E.n = n; E.nt = (n + T - 1) / T;
    E.first.resize((size_t)E.nt);
    for (int R = 0; R < E.nt; ++R) E.first[(size_t)R] = R;
}

// a block with rows row_lo .. row_hi whose first column is col: every row tile those rows fall in starts no later than col's tile
inline void llt_env_reach(std::vector<int32_t> &first, int T, int row_lo, int row_hi, int col)
{
    for (int R = row_lo / T; R <= row_hi / T; ++R) first[(size_t)R] = std::min(first[(size_t)R], (int32_t)(col / T));
}

// first[] is finished: live, launches and the image; refuses as orbm_llt_env_plan does
inline int llt_env_finish(LltEnvPlan &E)
{
    if (E.n == 0) return ORBX_OK;
    int32_t counts[4];
    if (const int e = orbm_llt_env_plan(E.n, E.first.data(), nullptr, nullptr, nullptr, nullptr, nullptr, counts)) return e;
    E.live = counts[0]; E.launches = counts[3];
    E.image.assign(LltEnvView::words((size_t)E.nt, (size_t)counts[1]), 0);
    const LltEnvImage<int32_t> im(E.image.data(), E.nt);
    std::copy(E.first.begin(), E.first.end(), im.first);
    return orbm_llt_env_plan(E.n, E.first.data(), im.off, im.row_start, im.rows, nullptr, nullptr, counts);
}
