"""ctypes mirror of the pose-only optimisation (include/orbslam_hip.h: orbm_pose_optimization, orbm_frame_pose_optimization,
orbm_pose_optimization_batch) -- Optimizer::PoseOptimization (src/Optimizer.cc:264-476) on the device -- and of the bundle of
Optimizer::PoseOptimizationNR (include/fem_hip.h: orbm_pose_optimization_nr, orbm_pose_optimization_nr_batch)."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr
from .extractor import KP_DTYPE


class PoseCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("nlevels", C.c_int32), ("inv_level_sigma2", C.c_void_p)]


class PoseStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4), ("ninitial", C.c_int32),
                ("chi2", C.c_double), ("q", C.c_double * 4), ("t", C.c_double * 3)]


def _camera(cam, inv_level_sigma2):
    inv = np.ascontiguousarray(inv_level_sigma2, np.float32)
    c = PoseCamera(*[float(v) for v in cam[:5]], len(inv), inv.ctypes.data)
    c._keep = inv
    return c


def _kps(kps_xy, octave):
    k = np.zeros(len(octave), KP_DTYPE)
    xy = np.asarray(kps_xy, np.float32).reshape(-1, 2)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], np.asarray(octave, np.int32)
    return k


def pose_optimization(kps_xy, octave, uright, has_mp, mp_pos, cam, inv_level_sigma2, Tcw, frame=None):
    """One PoseOptimization call.  kps_xy[n, 2] / octave[n] = mvKeysUn, uright[n] = mvuRight (None: monocular), has_mp[n],
    mp_pos[n, 3], cam = (fx, fy, cx, cy, mbf), Tcw = mTcw.  With `frame` (a matcher.Frame / orbm_frame handle on the same
    keypoints) kps_xy / octave / uright are not sent: the call reads them from the resident frame.
    Returns (ngood, Tcw_out float32[4, 4], outlier uint8[n] (0 where has_mp is not set), PoseStats)."""
    L = lib()
    has_mp = np.ascontiguousarray(has_mp, np.uint8)
    n = len(has_mp)
    mp = np.ascontiguousarray(mp_pos, np.float32).reshape(n, 3)
    Tin = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    Tout = np.zeros(16, np.float32)
    outlier = np.zeros(n, np.uint8)
    ng = C.c_int(0)
    st = PoseStats()
    c = _camera(cam, inv_level_sigma2)
    if frame is not None:
        h = frame._h if hasattr(frame, "_h") else frame
        check(L.orbm_frame_pose_optimization(h, ptr(has_mp), ptr(mp), C.byref(c), ptr(Tin), ptr(Tout), ptr(outlier), C.byref(ng),
                                             C.byref(st)))
    else:
        k = _kps(kps_xy, octave)
        ur = None if uright is None else ptr(np.ascontiguousarray(uright, np.float32))
        check(L.orbm_pose_optimization(ptr(k), ur, n, ptr(has_mp), ptr(mp), C.byref(c), ptr(Tin), ptr(Tout), ptr(outlier), C.byref(ng),
                                       C.byref(st)))
    return ng.value, Tout.reshape(4, 4), outlier, st


def pose_optimization_batch(problems, cam, inv_level_sigma2):
    """B problems in one launch (host arrays).  problems: list of dicts with kp_xy, octave, uright (or None), has_mp, mp_pos, Tcw.
    Returns a list of (ngood, Tcw_out, outlier, PoseStats) as pose_optimization returns them."""
    L = lib()
    B = len(problems)
    sizes = [len(p["has_mp"]) for p in problems]
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    k = np.concatenate([_kps(p["kp_xy"], p["octave"]) for p in problems]) if B else np.zeros(0, KP_DTYPE)
    ur = np.concatenate([np.full(s, -1, np.float32) if p["uright"] is None else np.asarray(p["uright"], np.float32)
                         for p, s in zip(problems, sizes)])
    has = np.ascontiguousarray(np.concatenate([np.asarray(p["has_mp"], np.uint8) for p in problems]))
    mp = np.ascontiguousarray(np.concatenate([np.asarray(p["mp_pos"], np.float32).reshape(-1, 3) for p in problems]))
    Tin = np.ascontiguousarray(np.stack([np.asarray(p["Tcw"], np.float32).reshape(16) for p in problems]))
    Tout = np.zeros((B, 16), np.float32)
    outlier = np.zeros(len(has), np.uint8)
    ng = np.zeros(B, np.int32)
    st = (PoseStats * max(B, 1))()
    c = _camera(cam, inv_level_sigma2)
    check(L.orbm_pose_optimization_batch(ptr(k), ptr(ur), ptr(off), B, ptr(has), ptr(mp), C.byref(c), ptr(Tin), ptr(Tout), ptr(outlier),
                                         ptr(ng), st, 0, None))
    return [(int(ng[p]), Tout[p].reshape(4, 4), outlier[off[p]:off[p + 1]], st[p]) for p in range(B)]


def _dptr(a):
    return None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else int(a)


def pose_optimization_batch_device(kps, uright, kp_off, batch, has_mp, mp_pos, cam, inv_level_sigma2, Tcw_in, Tcw_out, outlier, ngood,
                                   stats=None, stream=None):
    """B problems in one launch on device arrays (is_device = 1): every array argument is a device pointer or a tensor on the
    device -- kps orbx_keypoint[total], uright float[total] (None: every edge monocular), kp_off int32[B + 1], has_mp uint8[total],
    mp_pos float[total][3], Tcw_in / Tcw_out float[B][16], outlier uint8[total] (written only where has_mp), ngood int32[B],
    stats orbm_pose_stats[B] (PoseStats bytes, or None).  cam = (fx, fy, cx, cy, mbf) and inv_level_sigma2 are host values.
    Only enqueues the launch on `stream` (a raw hipStream_t, None: the null stream); a problem the kernel rejects gets
    ngood[p] < 0 and no other output."""
    L = lib()
    c = _camera(cam, inv_level_sigma2)
    check(L.orbm_pose_optimization_batch(_dptr(kps), _dptr(uright), _dptr(kp_off), int(batch), _dptr(has_mp), _dptr(mp_pos), C.byref(c),
                                         _dptr(Tcw_in), _dptr(Tcw_out), _dptr(outlier), _dptr(ngood), _dptr(stats), 1, _dptr(stream)))


# ---- Optimizer::PoseOptimizationNR's bundle on the device (include/fem_hip.h: orbm_pose_optimization_nr, ..._batch)

class PoseNRGraph(C.Structure):
    _fields_ = [("npoints", C.c_int32), ("nkf", C.c_int32), ("nedges", C.c_int32), ("reserved", C.c_int32),
                ("Tcw", C.c_void_p), ("kf_Tcw", C.c_void_p), ("points", C.c_void_p), ("e_point", C.c_void_p), ("e_cam", C.c_void_p),
                ("e_obs", C.c_void_p), ("e_inv_sigma2", C.c_void_p), ("e_cam_k", C.c_void_p)]


class PoseNRResult(C.Structure):
    _fields_ = [("Tcw", C.c_float * 16), ("points_out", C.c_void_p), ("outlier", C.c_void_p), ("ngood", C.c_int32), ("reserved", C.c_int32)]


class PoseNRStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4), ("nresults", C.c_int32),
                ("results", C.c_int32 * 40), ("trial_capacity", C.c_int32), ("ntrials", C.c_int32), ("trial_overflow", C.c_int32),
                ("reserved", C.c_int32), ("trial_log", C.c_void_p), ("q", C.c_double * 4), ("t", C.c_double * 3), ("points", C.c_void_p)]


# orbm_pose_nr_trial (the fields of orbslam_hip::PoseOptimizationNR_fem::Trial)
NR_TRIAL_DTYPE = np.dtype([("sE", "<f4"), ("nsE", "<f4"), ("tempChi", "<f8"), ("currentChi", "<f8"), ("rho", "<f8"), ("lam", "<f8"),
                           ("qmax", "<i4"), ("acc", "<i4")], align=True)
NR_TRIAL_CAPACITY = 400         # 4 rounds x 10 iterations x 10 trials


def _nr_graph(graph):
    """The ctypes struct of a flat graph (dict: Tcw[16], kf_Tcw[nkf, 16], points[n, 3], e_point, e_cam, e_obs[ne, 2], e_inv_sigma2[ne],
    e_cam_k[ne, 4]); the converted arrays stay alive with it."""
    a = {"Tcw": np.ascontiguousarray(graph["Tcw"], np.float32).reshape(16),
         "kf_Tcw": np.ascontiguousarray(graph["kf_Tcw"], np.float32).reshape(-1, 16),
         "points": np.ascontiguousarray(graph["points"], np.float32).reshape(-1, 3),
         "e_point": np.ascontiguousarray(graph["e_point"], np.int32), "e_cam": np.ascontiguousarray(graph["e_cam"], np.int32),
         "e_obs": np.ascontiguousarray(graph["e_obs"], np.float32).reshape(-1, 2),
         "e_inv_sigma2": np.ascontiguousarray(graph["e_inv_sigma2"], np.float32),
         "e_cam_k": np.ascontiguousarray(graph["e_cam_k"], np.float32).reshape(-1, 4)}
    ne = len(a["e_point"])
    if not (len(a["e_cam"]) == len(a["e_obs"]) == len(a["e_inv_sigma2"]) == len(a["e_cam_k"]) == ne):
        raise ValueError("the per-edge arrays of the graph differ in length")
    g = PoseNRGraph(len(a["points"]), len(a["kf_Tcw"]), ne, 0, *[a[k].ctypes.data for k in ("Tcw", "kf_Tcw", "points", "e_point", "e_cam",
                                                                                             "e_obs", "e_inv_sigma2", "e_cam_k")])
    g._keep = a
    return g


def _nr_buffers(n, want_stats):
    res = PoseNRResult()
    pts = np.zeros((n, 3), np.float32); outlier = np.zeros(n, np.uint8)
    res.points_out, res.outlier = pts.ctypes.data, outlier.ctypes.data
    st = log = ptsd = None
    if want_stats:
        st = PoseNRStats()
        log = np.zeros(NR_TRIAL_CAPACITY, NR_TRIAL_DTYPE); ptsd = np.zeros((n, 3), np.float64)
        st.trial_capacity, st.trial_log, st.points = len(log), log.ctypes.data, ptsd.ctypes.data
    return res, pts, outlier, st, log, ptsd


def _nr_collect(res, pts, outlier, st, log, ptsd):
    out = (int(res.ngood), np.array(res.Tcw, np.float32).reshape(4, 4), pts, outlier)
    if st is None:
        return out
    nlog = min(st.ntrials, st.trial_capacity)
    stats = {"rounds": st.rounds, "iterations": np.array(st.iterations[:]), "trials_per_round": np.array(st.trials[:]),
             "results": np.array(st.results[:st.nresults], np.int32), "ntrials": st.ntrials, "trial_overflow": st.trial_overflow,
             "trials": log[:nlog].copy(), "q": np.array(st.q[:]), "t": np.array(st.t[:]), "X": ptsd}
    return out + (stats,)


def _model(fea):
    h = fea._h if hasattr(fea, "_h") else fea
    return h.value if isinstance(h, C.c_void_p) else h


def pose_optimization_nr(fea, graph, want_stats=False):
    """Optimizer::PoseOptimizationNR's non-linear optimisation in one launch.  fea: a fem.FEA2 of ONE mesh, assembled, with the Dirichlet
    penalty and trial_setup made for len(graph["points"]) points (None for a graph of fewer than 3 points).  Returns (ngood,
    Tcw float32[4, 4], points float32[n, 3], outlier uint8[n]) and, with want_stats, a dict: rounds, iterations, trials_per_round,
    results, ntrials, trial_overflow, trials[NR_TRIAL_DTYPE], q, t, X (the final estimates in double)."""
    g = _nr_graph(graph)
    bufs = _nr_buffers(g.npoints, want_stats)
    check(lib().orbm_pose_optimization_nr(_model(fea), C.byref(g), C.byref(bufs[0]), None if bufs[3] is None else C.byref(bufs[3])))
    return _nr_collect(*bufs)


def pose_optimization_nr_batch(feas, graphs, want_stats=False):
    """B problems in one launch (host arrays), one workgroup each; feas[k] belongs to graphs[k].  Returns a list of what
    pose_optimization_nr returns."""
    B = len(graphs)
    if len(feas) != B:
        raise ValueError("one model per graph")
    gs = [_nr_graph(g) for g in graphs]
    bufs = [_nr_buffers(g.npoints, want_stats) for g in gs]
    models = (C.c_void_p * max(B, 1))(*[_model(f) for f in feas])
    garr = (PoseNRGraph * max(B, 1))(*gs)
    rarr = (PoseNRResult * max(B, 1))(*[b[0] for b in bufs])
    sarr = (PoseNRStats * max(B, 1))(*[b[3] for b in bufs]) if want_stats else None
    check(lib().orbm_pose_optimization_nr_batch(models, garr, B, rarr, sarr))
    return [_nr_collect(rarr[k], bufs[k][1], bufs[k][2], sarr[k] if want_stats else None, bufs[k][4], bufs[k][5]) for k in range(B)]
