"""Optimizer::OptimizeEssentialGraph on the device (include/orbslam_hip.h, orbm_essential_graph): the struct mirrors of
the C ABI, the flat graph from numpy arrays, the call and its host-only plan; and the same two for the essential graph of a long
session on the tile-envelope solver (orbm_essential_graph_env)."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr
from .bundle import BA_TRIAL_DTYPE

_vp = C.c_void_p
ITERATIONS = 20             # ORBM_EG_ITERATIONS
LAMBDA_INIT = 1e-16         # setUserLambdaInit
TRIAL_CAPACITY = 10 * 64


class EgGraph(C.Structure):
    _fields_ = [("nvert", C.c_int32), ("ncorr", C.c_int32), ("nnc", C.c_int32), ("nedges", C.c_int32), ("npoints", C.c_int32),
                ("fix_scale", C.c_int32), ("poses", _vp), ("corrected", _vp), ("corrected_sim3", _vp), ("noncorrected", _vp),
                ("noncorrected_sim3", _vp), ("fixed", _vp), ("e_v0", _vp), ("e_v1", _vp), ("e_kind", _vp), ("points", _vp), ("p_ref", _vp)]


class EgOptions(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("lambda_init", C.c_double)]


class EgResult(C.Structure):
    _fields_ = [("poses", _vp), ("points", _vp)]


class EgStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("nresults", C.c_int32), ("results", C.c_int32 * 64),
                ("trial_capacity", C.c_int32), ("ntrials", C.c_int32), ("trial_overflow", C.c_int32), ("trial_log", _vp),
                ("estimates", _vp), ("chi2", _vp)]


def default_options(iterations=ITERATIONS, lambda_init=LAMBDA_INIT):
    """ORBM_EG_OPTIONS_DEFAULT"""
    return EgOptions(iterations, 0, lambda_init)


def make_graph(poses, fixed, e_v0, e_v1, e_kind, fix_scale, corrected=None, corrected_sim3=None, noncorrected=None, noncorrected_sim3=None,
               points=None, p_ref=None):
    """The arrays of orbm_eg_graph as the C ABI takes them (contiguous, the ABI's types), in a dict that keeps them alive.  corrected /
    noncorrected default to -1 everywhere (no table entry)."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    nv = len(poses)

    def index(a):
        return np.full(nv, -1, np.int32) if a is None else np.ascontiguousarray(a, np.int32)

    def table(a):
        return np.zeros((0, 8)) if a is None else np.ascontiguousarray(a, np.float64).reshape(-1, 8)
    return {"poses": poses, "fixed": np.ascontiguousarray(fixed, np.uint8), "e_v0": np.ascontiguousarray(e_v0, np.int32),
            "e_v1": np.ascontiguousarray(e_v1, np.int32), "e_kind": np.ascontiguousarray(e_kind, np.uint8), "fix_scale": int(bool(fix_scale)),
            "corrected": index(corrected), "corrected_sim3": table(corrected_sim3), "noncorrected": index(noncorrected),
            "noncorrected_sim3": table(noncorrected_sim3),
            "points": np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3),
            "p_ref": np.zeros(0, np.int32) if p_ref is None else np.ascontiguousarray(p_ref, np.int32)}


def c_graph(g):
    def p(a):
        return None if a is None or a.size == 0 else ptr(a)
    return EgGraph(len(g["poses"]), len(g["corrected_sim3"]), len(g["noncorrected_sim3"]), len(g["e_v0"]), len(g["points"]), g["fix_scale"],
                   p(g["poses"]), p(g["corrected"]), p(g["corrected_sim3"]), p(g["noncorrected"]), p(g["noncorrected_sim3"]), p(g["fixed"]),
                   p(g["e_v0"]), p(g["e_v1"]), p(g["e_kind"]), p(g["points"]), p(g["p_ref"]))


def plan(g, env=False):
    """orbm_eg_plan: the vertex classes, the rows and the index lists the call would use (host only).  env: orbm_eg_env_plan, which
    adds first (the tile envelope), row_tiles, live_tiles and launches (of one solve)."""
    entry = lib().orbm_eg_env_plan if env else lib().orbm_eg_plan
    cg = c_graph(g)
    nv = len(g["poses"])
    counts = np.zeros(6 if env else 3, np.int32)
    first = [np.zeros(1, np.int32)] if env else []
    check(entry(C.byref(cg), None, None, None, None, None, None, None, *([None] if env else []), ptr(counts)))
    nve, npairs, npe = (int(c) for c in counts[:3])
    if env:
        first = [np.zeros(max(int(counts[3]), 1), np.int32)]
    out = {"vertex_class": np.zeros(max(nv, 1), np.int32), "row": np.zeros(max(nv, 1), np.int32), "vert_edge_start": np.zeros(nv + 1, np.int32),
           "vert_edges": np.zeros(max(nve, 1), np.int32), "pair_start": np.zeros(npairs + 1, np.int32),
           "pair_v": np.zeros((max(npairs, 1), 2), np.int32), "pair_edges": np.zeros(max(npe, 1), np.int32)}
    check(entry(C.byref(cg), *(ptr(out[k]) for k in ("vertex_class", "row", "vert_edge_start", "vert_edges", "pair_start", "pair_v", "pair_edges")),
                *(ptr(a) for a in first), ptr(counts)))
    if env:
        out.update(first=first[0][:counts[3]], row_tiles=int(counts[3]), live_tiles=int(counts[4]), launches=int(counts[5]))
    out["vertex_class"] = out["vertex_class"][:nv]; out["row"] = out["row"][:nv]
    out["vert_edges"] = out["vert_edges"][:nve]; out["pair_v"] = out["pair_v"][:npairs]; out["pair_edges"] = out["pair_edges"][:npe]
    return out


def plan_env(g):
    """orbm_eg_env_plan: plan(g) under the envelope entry's limits, plus first, row_tiles, live_tiles and launches."""
    return plan(g, env=True)


def optimize_env(g, iterations=ITERATIONS, lambda_init=LAMBDA_INIT, want_stats=False):
    """orbm_essential_graph_env: optimize() for up to 4,096 free keyframes, on the tile-envelope solver.  List the keyframes by
    ascending mnId: the order decides the envelope (plan_env shows what it costs)."""
    return optimize(g, iterations, lambda_init, want_stats, env=True)


def optimize(g, iterations=ITERATIONS, lambda_init=LAMBDA_INIT, want_stats=False, env=False):
    """orbm_essential_graph (env: orbm_essential_graph_env).  Returns a dict: poses [nvert][16], points [npoints][3], waits, and with want_stats the fields of
    orbm_eg_stats (iterations, trials, results, ntrials, trial_overflow, trial_log, estimates [nvert][8], chi2 [nedges])."""
    L = lib()
    cg = c_graph(g)
    opt = default_options(iterations, lambda_init)
    nv, npts, ne = len(g["poses"]), len(g["points"]), len(g["e_v0"])
    poses = np.zeros((max(nv, 1), 16), np.float32); points = np.zeros((max(npts, 1), 3), np.float32)
    res = EgResult(ptr(poses), ptr(points))
    st = None
    if want_stats:
        log = np.zeros(TRIAL_CAPACITY, BA_TRIAL_DTYPE)
        est = np.zeros((max(nv, 1), 8)); chi2 = np.zeros(max(ne, 1))
        st = EgStats()
        st.trial_capacity = TRIAL_CAPACITY
        st.trial_log, st.estimates, st.chi2 = (ptr(a).value for a in (log, est, chi2))
    check((L.orbm_essential_graph_env if env else L.orbm_essential_graph)(C.byref(cg), C.byref(opt), C.byref(res), C.byref(st) if st is not None else None))
    out = {"poses": poses[:nv], "points": points[:npts], "waits": L.orbm_debug_last_eg_waits()}
    if want_stats:
        out.update(iterations=st.iterations, trials=st.trials, results=list(st.results[:min(st.nresults, 64)]), ntrials=st.ntrials,
                   trial_overflow=st.trial_overflow, trial_log=log[:min(st.ntrials, TRIAL_CAPACITY)], estimates=est[:nv], chi2=chi2[:ne])
    return out
