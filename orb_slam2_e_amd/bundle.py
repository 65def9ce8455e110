"""Optimizer::LocalBundleAdjustment / Optimizer::BundleAdjustment on the device (include/orbslam_hip.h, orbm_bundle_adjustment;
DESIGN.md 24): the struct mirrors of the C ABI, the flat graph from numpy arrays, and the two calls.  The same for a whole map of up
to 512 keyframes (orbm_global_bundle_adjustment), of up to 4,096 keyframes on the tile envelope
(orbm_global_bundle_adjustment_env), and the tiled Cholesky solves under them on torch device tensors."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr

_vp = C.c_void_p
HUBER_MONO_LOCAL = float(np.float32(np.sqrt(5.991)))        # (float)sqrt(5.991)
HUBER_MONO_GLOBAL = float(np.float32(np.sqrt(5.99)))        # BundleAdjustment: 5.99
HUBER_STEREO = float(np.float32(np.sqrt(7.815)))


class BaGraph(C.Structure):
    _fields_ = [("nfree", C.c_int32), ("nfixed", C.c_int32), ("npoints", C.c_int32), ("nedges", C.c_int32), ("poses", _vp), ("fixed", _vp),
                ("points", _vp), ("e_point", _vp), ("e_cam", _vp), ("e_obs", _vp), ("e_inv_sigma2", _vp), ("e_cam_k", _vp)]


class BaOptions(C.Structure):
    _fields_ = [("nrounds", C.c_int32), ("iterations", C.c_int32 * 2), ("robust_round0", C.c_int32), ("classify", C.c_int32),
                ("reserved", C.c_int32), ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("chi2_mono", C.c_double),
                ("chi2_stereo", C.c_double)]


class BaResult(C.Structure):
    _fields_ = [("poses", _vp), ("points", _vp), ("erase", _vp), ("not_included", _vp), ("stopped", C.c_int32)]


class BaStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("nresults", C.c_int32),
                ("results", C.c_int32 * 128), ("trial_capacity", C.c_int32), ("ntrials", C.c_int32), ("trial_overflow", C.c_int32),
                ("trial_log", _vp), ("poses", _vp), ("points", _vp), ("chi2", _vp), ("level", _vp)]


# orbm_ba_trial
BA_TRIAL_DTYPE = np.dtype([("tempChi", "<f8"), ("currentChi", "<f8"), ("rho", "<f8"), ("lam", "<f8"), ("scale", "<f8"), ("round", "<i4"),
                           ("qmax", "<i4"), ("accepted", "<i4"), ("ok2", "<i4")], align=True)
TRIAL_CAPACITY = 10 * 128


def local_options():
    """ORBM_BA_OPTIONS_LOCAL"""
    return BaOptions(2, (5, 10), 1, 1, 0, HUBER_MONO_LOCAL, HUBER_STEREO, 5.991, 7.815)


def global_options(iterations=5, robust=True):
    """ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust)"""
    return BaOptions(1, (iterations, 0), 1 if robust else 0, 0, 0, HUBER_MONO_GLOBAL, HUBER_STEREO, 5.99, 7.815)


def make_graph(poses, nfree, points, e_point, e_cam, e_obs, e_inv_sigma2, e_cam_k, fixed=None):
    """The arrays of orbm_ba_graph as the C ABI takes them (float32 / int32, contiguous), in a dict that keeps them alive."""
    g = {"poses": np.ascontiguousarray(poses, np.float32).reshape(-1, 16), "points": np.ascontiguousarray(points, np.float32).reshape(-1, 3),
         "e_point": np.ascontiguousarray(e_point, np.int32), "e_cam": np.ascontiguousarray(e_cam, np.int32),
         "e_obs": np.ascontiguousarray(e_obs, np.float32).reshape(-1, 3), "e_inv_sigma2": np.ascontiguousarray(e_inv_sigma2, np.float32),
         "e_cam_k": np.ascontiguousarray(e_cam_k, np.float32).reshape(-1, 5), "nfree": int(nfree),
         "fixed": None if fixed is None else np.ascontiguousarray(fixed, np.uint8)}
    return g


def c_graph(g):
    def p(a):
        return None if a is None or a.size == 0 else ptr(a)
    return BaGraph(g["nfree"], len(g["poses"]) - g["nfree"], len(g["points"]), len(g["e_point"]), p(g["poses"]), p(g["fixed"]), p(g["points"]),
                   p(g["e_point"]), p(g["e_cam"]), p(g["e_obs"]), p(g["e_inv_sigma2"]), p(g["e_cam_k"]))


def plan(g):
    """orbm_ba_plan: the vertex classes and the index lists the call would use (host only)."""
    return _plan(g, lib().orbm_ba_plan)


def plan_global(g):
    """orbm_global_ba_plan: the same lists under the limits of orbm_global_bundle_adjustment (512 free keyframes)."""
    return _plan(g, lib().orbm_global_ba_plan)


def _plan(g, entry):
    cg = c_graph(g)
    nfree, npose, npts = g["nfree"], len(g["poses"]), len(g["points"])
    counts = np.zeros(2, np.int32)
    check(entry(C.byref(cg), None, None, None, None, None, None, ptr(counts)))
    out = {"pose_class": np.zeros(npose, np.int32), "point_class": np.zeros(npts, np.int32), "pose_edge_start": np.zeros(nfree + 1, np.int32),
           "pose_edges": np.zeros(max(int(counts[0]), 1), np.int32), "block_start": np.zeros(nfree * (nfree + 1) // 2 + 1, np.int32),
           "block_entries": np.zeros((max(int(counts[1]), 1), 3), np.int32)}
    check(entry(C.byref(cg), *(ptr(out[k]) if out[k].size else None for k in
                               ("pose_class", "point_class", "pose_edge_start", "pose_edges", "block_start", "block_entries")), ptr(counts)))
    out["pose_edges"] = out["pose_edges"][:counts[0]]
    out["block_entries"] = out["block_entries"][:counts[1]]
    return out


def plan_global_env(g):
    """orbm_global_ba_env_plan (host only): the vertex classes and pose -> edge lists of plan(), the COMPACT block list -- blk_i1,
    blk_i2, block_start [listed + 1], block_entries, the non-empty upper blocks sorted by (i1, i2) -- and round 0's tile envelope:
    first [row tiles], live_tiles, launches (of one solve).  Limits: 4,096 free keyframes, 8,192 live tiles."""
    cg = c_graph(g)
    nfree, npose, npts = g["nfree"], len(g["poses"]), len(g["points"])
    counts = np.zeros(6, np.int32)
    entry = lib().orbm_global_ba_env_plan
    check(entry(C.byref(cg), *([None] * 9), ptr(counts)))
    out = {"pose_class": np.zeros(npose, np.int32), "point_class": np.zeros(npts, np.int32), "pose_edge_start": np.zeros(nfree + 1, np.int32),
           "pose_edges": np.zeros(max(int(counts[0]), 1), np.int32), "blk_i1": np.zeros(max(int(counts[2]), 1), np.int32),
           "blk_i2": np.zeros(max(int(counts[2]), 1), np.int32), "block_start": np.zeros(int(counts[2]) + 1, np.int32),
           "block_entries": np.zeros((max(int(counts[1]), 1), 3), np.int32), "first": np.zeros(max(int(counts[3]), 1), np.int32)}
    check(entry(C.byref(cg), *(ptr(out[k]) if out[k].size else None for k in
                               ("pose_class", "point_class", "pose_edge_start", "pose_edges", "blk_i1", "blk_i2", "block_start",
                                "block_entries", "first")), ptr(counts)))
    out["pose_edges"] = out["pose_edges"][:counts[0]]
    out["block_entries"] = out["block_entries"][:counts[1]]
    out["blk_i1"], out["blk_i2"], out["first"] = out["blk_i1"][:counts[2]], out["blk_i2"][:counts[2]], out["first"][:counts[3]]
    out.update(live_tiles=int(counts[4]), launches=int(counts[5]))
    return out


def run(g, options, stop_flag=None, want_stats=False):
    """orbm_bundle_adjustment (up to 64 free keyframes).  See _run for the arguments and the result."""
    return _run(g, options, stop_flag, want_stats, lib().orbm_bundle_adjustment)


def run_global(g, options, stop_flag=None, want_stats=False):
    """orbm_global_bundle_adjustment: the same call for up to 512 free keyframes; its reduced system is always solved by the tiled
    multi-workgroup Cholesky (llt_solve_device), which gives run()'s bytes wherever both accept the graph."""
    return _run(g, options, stop_flag, want_stats, lib().orbm_global_bundle_adjustment)


def run_global_env(g, options, stop_flag=None, want_stats=False):
    """orbm_global_bundle_adjustment_env: the same call for up to 4,096 free keyframes, LISTED BY ASCENDING mnId; its reduced system
    lives in the live tiles of its tile envelope and is solved by the envelope Cholesky (llt_env_solve_device), which gives
    run_global()'s numbers wherever both accept the graph."""
    return _run(g, options, stop_flag, want_stats, lib().orbm_global_bundle_adjustment_env)


def _run(g, options, stop_flag, want_stats, entry):
    """Either bundle-adjustment entry.  stop_flag: a numpy uint8 array of one element (pbStopFlag) or None.  Returns a dict: poses
    [nfree][16], points [npoints][3], erase [nedges] (with classify), not_included [npoints], stopped, and with want_stats the
    fields of orbm_ba_stats."""
    L = lib()
    cg = c_graph(g)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    poses = np.zeros((max(nfree, 1), 16), np.float32); points = np.zeros((max(npts, 1), 3), np.float32)
    erase = np.zeros(max(ne, 1), np.uint8); notinc = np.zeros(max(npts, 1), np.uint8)
    res = BaResult(ptr(poses), ptr(points), ptr(erase), ptr(notinc), 0)
    st = None
    if want_stats:
        log = np.zeros(TRIAL_CAPACITY, BA_TRIAL_DTYPE)
        pd = np.zeros((max(nfree, 1), 7)); xd = np.zeros((max(npts, 1), 3)); chi2 = np.zeros(max(ne, 1)); level = np.zeros(max(ne, 1), np.uint8)
        st = BaStats()
        st.trial_capacity = TRIAL_CAPACITY
        st.trial_log, st.poses, st.points, st.chi2, st.level = (ptr(a).value for a in (log, pd, xd, chi2, level))
    check(entry(C.byref(cg), C.byref(options), None if stop_flag is None else ptr(stop_flag), C.byref(res),
                C.byref(st) if st is not None else None))
    out = {"poses": poses[:nfree], "points": points[:npts], "erase": erase[:ne], "not_included": notinc[:npts], "stopped": res.stopped,
           "waits": L.orbm_debug_last_ba_waits()}
    if want_stats:
        out.update(rounds=st.rounds, iterations=list(st.iterations), trials=list(st.trials), results=list(st.results[:min(st.nresults, 128)]),
                   ntrials=st.ntrials, trial_overflow=st.trial_overflow, trial_log=log[:min(st.ntrials, TRIAL_CAPACITY)], poses_d=pd[:nfree],
                   points_d=xd[:npts], chi2=chi2[:ne], level=level[:ne])
    return out


def local_bundle_adjustment(g, stop_flag=None, want_stats=False):
    """Optimizer::LocalBundleAdjustment on the flattened graph: optimize(5) with Huber, the level pass, optimize(10), vToErase."""
    return run(g, local_options(), stop_flag, want_stats)


def bundle_adjustment(g, iterations=5, robust=True, stop_flag=None, want_stats=False):
    """Optimizer::BundleAdjustment on the flattened graph: one round of optimize(iterations); not_included marks the points left out."""
    return run(g, global_options(iterations, robust), stop_flag, want_stats)


def global_bundle_adjustment(g, iterations=10, robust=False, stop_flag=None, want_stats=False):
    """Optimizer::GlobalBundleAdjustemnt on the flattened graph of a whole map, up to 512 keyframes (LoopClosing runs it with 10
    iterations and bRobust = false): bundle_adjustment through orbm_global_bundle_adjustment."""
    return run_global(g, global_options(iterations, robust), stop_flag, want_stats)


def global_bundle_adjustment_env(g, iterations=10, robust=False, stop_flag=None, want_stats=False):
    """Optimizer::GlobalBundleAdjustemnt on the flattened graph of the map of a long session, up to 4,096 keyframes listed by
    ascending mnId: global_bundle_adjustment through orbm_global_bundle_adjustment_env."""
    return run_global_env(g, global_options(iterations, robust), stop_flag, want_stats)


def llt_tile():
    """orbm_llt_tile: the tile edge of the tiled Cholesky solve."""
    return lib().orbm_llt_tile()


def llt_solve_device(S_dev, b_dev, x_dev, ok_dev, stream=None):
    """orbm_llt_solve_dev on torch device tensors, asynchronous on `stream` (a torch.cuda.Stream; None: the current one).  S_dev:
    float64 [n][n], contiguous, whose element [j][i] is entry (row i, column j) of the matrix -- only i >= j is read; it comes back
    with L in that triangle and scratch in the other.  b_dev, x_dev: float64 [n]; ok_dev: int32 [1].  Nothing is waited for."""
    import torch
    n = int(b_dev.numel())
    for t, dt, numel in ((S_dev, torch.float64, n * n), (b_dev, torch.float64, n), (x_dev, torch.float64, n), (ok_dev, torch.int32, 1)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == numel):
            raise ValueError("llt_solve_device: contiguous device tensors float64 [n][n], [n], [n] and int32 [1]")
    st = (stream if stream is not None else torch.cuda.current_stream(S_dev.device)).cuda_stream
    check(lib().orbm_llt_solve_dev(n, S_dev.data_ptr(), b_dev.data_ptr(), x_dev.data_ptr(), ok_dev.data_ptr(), st))


def llt_env_plan(n, first):
    """orbm_llt_env_plan (host only): what the envelope solve does for n rows and first[] (the first live column tile of every row
    tile).  A dict: off [nt + 1], row_start [nt + 1], rows, trail_start [nt + 1], trail [][2], live_tiles, launches, and `device`,
    the int32 image orbm_llt_env_solve_dev reads on the device (first, off, row_start, rows)."""
    first = np.ascontiguousarray(first, np.int32)
    nt = len(first)
    counts = np.zeros(4, np.int32)
    check(lib().orbm_llt_env_plan(n, ptr(first), None, None, None, None, None, ptr(counts)))
    off, row_start, trail_start = (np.zeros(nt + 1, np.int32) for _ in range(3))
    rows, trail = np.zeros(max(int(counts[1]), 1), np.int32), np.zeros((max(int(counts[2]), 1), 2), np.int32)
    check(lib().orbm_llt_env_plan(n, ptr(first), ptr(off), ptr(row_start), ptr(rows), ptr(trail_start), ptr(trail), ptr(counts)))
    rows, trail = rows[:counts[1]], trail[:counts[2]]
    return {"first": first, "off": off, "row_start": row_start, "rows": rows, "trail_start": trail_start, "trail": trail,
            "live_tiles": int(counts[0]), "launches": int(counts[3]), "device": np.concatenate([first, off, row_start, rows])}


def llt_env_solve_device(first, plan_dev, A_dev, W_dev, b_dev, x_dev, ok_dev, stream=None):
    """orbm_llt_env_solve_dev on torch device tensors, asynchronous on `stream` (None: the current one).  first: host int32 [nt];
    plan_dev: llt_env_plan(...)["device"] as a device int32 tensor; A_dev: the live tiles, float64 [live][T][T] with element
    [tile][j][i] = entry (i, j) of the tile -- it comes back with L; W_dev: as many float64, scratch; b_dev, x_dev: float64 [n];
    ok_dev: int32 [1].  Nothing is waited for."""
    import torch
    first = np.ascontiguousarray(first, np.int32)
    n, T = int(b_dev.numel()), llt_tile()
    nt = (n + T - 1) // T
    if len(first) != nt:
        raise ValueError("llt_env_solve_device: first holds one entry per row tile")
    live = int(np.sum(np.arange(nt) - first + 1))
    for t, dt, numel in ((A_dev, torch.float64, live * T * T), (W_dev, torch.float64, live * T * T), (b_dev, torch.float64, n),
                         (x_dev, torch.float64, n), (ok_dev, torch.int32, 1), (plan_dev, torch.int32, None)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and (numel is None or t.numel() == numel)):
            raise ValueError("llt_env_solve_device: contiguous device tensors float64 [live][T][T] twice, [n], [n], int32 [1] and the plan")
    st = (stream if stream is not None else torch.cuda.current_stream(A_dev.device)).cuda_stream
    check(lib().orbm_llt_env_solve_dev(n, ptr(first), plan_dev.data_ptr(), A_dev.data_ptr(), W_dev.data_ptr(), b_dev.data_ptr(),
                                       x_dev.data_ptr(), ok_dev.data_ptr(), st))
