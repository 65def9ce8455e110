"""ctypes wrapper of tests/essential_graph_oracle.c, the CPU restatement of Optimizer::OptimizeEssentialGraph for orbm_essential_graph
(test infrastructure: never part of the product).  The C file is compiled on first use into a per-user cache directory
(tests/c_oracle.py).  It takes the graph dict of orb_slam2_e_amd.essential_graph.make_graph and returns the dict
orb_slam2_e_amd.essential_graph.optimize returns with want_stats, plus J0 / b0 (the Jacobians and the right-hand side of iteration 0)
and meas (the measurements Sji)."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "essential_graph_oracle.c")
_LIBS = {}
_vp = C.c_void_p

TRIAL_DTYPE = np.dtype([("tempChi", "<f8"), ("currentChi", "<f8"), ("rho", "<f8"), ("lam", "<f8"), ("scale", "<f8"), ("round", "<i4"),
                        ("qmax", "<i4"), ("accepted", "<i4"), ("ok2", "<i4")], align=True)
CAP = 640


class Graph(C.Structure):
    _fields_ = [("nvert", C.c_int32), ("ncorr", C.c_int32), ("nnc", C.c_int32), ("nedges", C.c_int32), ("npoints", C.c_int32),
                ("fix_scale", C.c_int32), ("poses", _vp), ("corrected", _vp), ("corrected_sim3", _vp), ("noncorrected", _vp),
                ("noncorrected_sim3", _vp), ("fixed", _vp), ("e_v0", _vp), ("e_v1", _vp), ("e_kind", _vp), ("points", _vp), ("p_ref", _vp)]


class Options(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("lambda_init", C.c_double)]


class Out(C.Structure):
    _fields_ = [("poses", _vp), ("points", _vp), ("iterations", C.c_int32), ("trials", C.c_int32), ("nresults", C.c_int32),
                ("results", C.c_int32 * 64), ("trial_capacity", C.c_int32), ("ntrials", C.c_int32), ("trial_log", _vp), ("estimates", _vp),
                ("chi2", _vp), ("J0", _vp), ("b0", _vp), ("meas", _vp)]


def lib(flags=("-O2",)):
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(SRC, [os.path.join(_HERE, "g2o_restated.h")], (*flags, "-D_GNU_SOURCE")))
        L.ego_run.argtypes = [C.POINTER(Graph), C.POINTER(Options), C.POINTER(Out)]
        L.ego_run.restype = C.c_int
        L.ego_set_ulp.argtypes = [C.c_uint64]; L.ego_set_ulp.restype = None
        L.ego_sim3_log.argtypes = [_vp, _vp]; L.ego_sim3_log.restype = None
        L.ego_sim3_exp.argtypes = [_vp, _vp]; L.ego_sim3_exp.restype = None
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(_vp)


def sim3_exp(u):
    """Sim3(Vector7d) as [q xyzw, t, s]"""
    u = np.ascontiguousarray(u, np.float64); o = np.zeros(8)
    lib().ego_sim3_exp(_p(u), _p(o))
    return o


def sim3_log(S):
    S = np.ascontiguousarray(S, np.float64); o = np.zeros(7)
    lib().ego_sim3_log(_p(S), _p(o))
    return o


def run(g, iterations=20, lambda_init=1e-16, ulp_seed=0, flags=("-O2",), want_system=True):
    L = lib(flags)
    nv, npts, ne = len(g["poses"]), len(g["points"]), len(g["e_v0"])
    cg = Graph(nv, len(g["corrected_sim3"]), len(g["noncorrected_sim3"]), ne, npts, g["fix_scale"], _p(g["poses"]), _p(g["corrected"]),
               _p(g["corrected_sim3"]), _p(g["noncorrected"]), _p(g["noncorrected_sim3"]), _p(g["fixed"]), _p(g["e_v0"]), _p(g["e_v1"]),
               _p(g["e_kind"]), _p(g["points"]), _p(g["p_ref"]))
    poses = np.zeros((max(nv, 1), 16), np.float32); points = np.zeros((max(npts, 1), 3), np.float32)
    log = np.zeros(CAP, TRIAL_DTYPE); est = np.zeros((max(nv, 1), 8)); chi2 = np.zeros(max(ne, 1))
    J0 = np.zeros((max(ne, 1), 2, 7, 7)); b0 = np.zeros(7 * max(nv, 1)); meas = np.zeros((max(ne, 1), 8))
    o = Out()
    o.poses, o.points = poses.ctypes.data, points.ctypes.data
    o.trial_capacity = CAP
    o.trial_log, o.estimates, o.chi2, o.meas = (a.ctypes.data for a in (log, est, chi2, meas))
    if want_system:
        o.J0, o.b0 = J0.ctypes.data, b0.ctypes.data
    co = Options(iterations, 0, lambda_init)
    L.ego_set_ulp(ulp_seed)
    rc = L.ego_run(C.byref(cg), C.byref(co), C.byref(o))
    L.ego_set_ulp(0)
    assert rc == 0
    return {"poses": poses[:nv], "points": points[:npts], "iterations": o.iterations, "trials": o.trials,
            "results": list(o.results[:min(o.nresults, 64)]), "ntrials": o.ntrials, "trial_log": log[:min(o.ntrials, CAP)], "estimates": est[:nv],
            "chi2": chi2[:ne], "J0": J0[:ne], "b0": b0, "meas": meas[:ne]}
