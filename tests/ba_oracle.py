"""ctypes wrapper of tests/ba_oracle.c, the CPU restatement of Optimizer::LocalBundleAdjustment / BundleAdjustment for
orbm_bundle_adjustment (test infrastructure: never part of the product).  The C file is compiled on first use into a per-user cache
directory (tests/c_oracle.py).  It takes the graph dict of orb_slam2_e_amd.bundle.make_graph and returns the same dict
orb_slam2_e_amd.bundle.run returns with want_stats, plus nreads (stop-flag reads), lambda_init and chi2_round1_start."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "ba_oracle.c")
_LIBS = {}
_vp = C.c_void_p

TRIAL_DTYPE = np.dtype([("tempChi", "<f8"), ("currentChi", "<f8"), ("rho", "<f8"), ("lam", "<f8"), ("scale", "<f8"), ("round", "<i4"),
                        ("qmax", "<i4"), ("accepted", "<i4"), ("ok2", "<i4")], align=True)
CAP = 1280


class Graph(C.Structure):
    _fields_ = [("nfree", C.c_int32), ("nfixed", C.c_int32), ("npoints", C.c_int32), ("nedges", C.c_int32), ("poses", _vp), ("fixed", _vp),
                ("points", _vp), ("e_point", _vp), ("e_cam", _vp), ("e_obs", _vp), ("e_inv_sigma2", _vp), ("e_cam_k", _vp)]


class Options(C.Structure):
    _fields_ = [("nrounds", C.c_int32), ("iterations", C.c_int32 * 2), ("robust_round0", C.c_int32), ("classify", C.c_int32),
                ("reserved", C.c_int32), ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("chi2_mono", C.c_double),
                ("chi2_stereo", C.c_double)]


class Out(C.Structure):
    _fields_ = [("poses", _vp), ("points", _vp), ("erase", _vp), ("not_included", _vp), ("stopped", C.c_int32), ("rounds", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("nresults", C.c_int32), ("results", C.c_int32 * 128),
                ("trial_capacity", C.c_int32), ("ntrials", C.c_int32), ("nreads", C.c_int32), ("trial_log", _vp), ("poses_d", _vp),
                ("points_d", _vp), ("chi2", _vp), ("level", _vp), ("lambda_init", C.c_double * 2), ("chi2_round1_start", C.c_double)]


def lib(flags=("-O2",)):
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(SRC, [os.path.join(_HERE, "g2o_restated.h")], (*flags, "-D_GNU_SOURCE")))
        L.bao_run.argtypes = [C.POINTER(Graph), C.POINTER(Options), C.c_int, C.POINTER(Out)]
        L.bao_run.restype = C.c_int
        L.bao_set_ulp.argtypes = [C.c_uint64]; L.bao_set_ulp.restype = None
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(_vp)


def options(o):
    """from orb_slam2_e_amd.bundle.BaOptions (same fields)"""
    return Options(o.nrounds, tuple(o.iterations), o.robust_round0, o.classify, 0, o.huber_mono, o.huber_stereo, o.chi2_mono, o.chi2_stereo)


def run(g, opt, stop_at=0, ulp_seed=0, flags=("-O2",)):
    L = lib(flags)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    cg = Graph(nfree, len(g["poses"]) - nfree, npts, ne, _p(g["poses"]), _p(g["fixed"]), _p(g["points"]), _p(g["e_point"]), _p(g["e_cam"]),
               _p(g["e_obs"]), _p(g["e_inv_sigma2"]), _p(g["e_cam_k"]))
    poses = np.zeros((max(nfree, 1), 16), np.float32); points = np.zeros((max(npts, 1), 3), np.float32)
    erase = np.zeros(max(ne, 1), np.uint8); notinc = np.zeros(max(npts, 1), np.uint8)
    log = np.zeros(CAP, TRIAL_DTYPE); pd = np.zeros((max(nfree, 1), 7)); xd = np.zeros((max(npts, 1), 3)); chi2 = np.zeros(max(ne, 1))
    level = np.zeros(max(ne, 1), np.uint8)
    o = Out()
    o.poses, o.points, o.erase, o.not_included = (a.ctypes.data for a in (poses, points, erase, notinc))
    o.trial_capacity = CAP
    o.trial_log, o.poses_d, o.points_d, o.chi2, o.level = (a.ctypes.data for a in (log, pd, xd, chi2, level))
    co = options(opt)
    L.bao_set_ulp(ulp_seed)
    rc = L.bao_run(C.byref(cg), C.byref(co), stop_at, C.byref(o))
    L.bao_set_ulp(0)
    assert rc == 0
    return {"poses": poses[:nfree], "points": points[:npts], "erase": erase[:ne] if opt.classify else np.zeros(ne, np.uint8),
            "not_included": notinc[:npts], "stopped": o.stopped, "rounds": o.rounds, "iterations": list(o.iterations), "trials": list(o.trials),
            "results": list(o.results[:min(o.nresults, 128)]), "ntrials": o.ntrials, "trial_log": log[:min(o.ntrials, CAP)], "poses_d": pd[:nfree],
            "points_d": xd[:npts], "chi2": chi2[:ne], "level": level[:ne], "nreads": o.nreads, "lambda_init": list(o.lambda_init),
            "chi2_round1_start": o.chi2_round1_start}
