"""ctypes wrapper of tests/sim3_opt_oracle.c, the CPU restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1564-1624) on g2o's code
paths (test infrastructure: never part of the product).  The C file is compiled on first use into a per-user cache directory
(tests/c_oracle.py)."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sim3_opt_oracle.c")
_LIBS = {}


class Sim3(C.Structure):        # s3x_sim3: q = x y z w
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double)]

    def vec(self):
        return np.array(list(self.q) + list(self.t) + [self.s])


class Result(C.Structure):      # s3x_result = orbm_sim3_opt_result
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("nin", C.c_int32), ("nbad", C.c_int32),
                ("ncorrespondences", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("chi2", C.c_double)]

    def vec(self):
        return np.array(list(self.q) + list(self.t) + [self.s])


class Trace(C.Structure):       # s3x_trace
    _fields_ = [("small_rho", C.c_int32), ("eval_is_est", C.c_int32 * 2), ("H6max", C.c_double), ("b6", C.c_double), ("lambda0", C.c_double * 2),
                ("min_abs_rho", C.c_double), ("hit_limit", C.c_int32 * 2)]


def lib(flags=("-O2",)):
    """the restatement built with `flags` (always -ffp-contract=off -fno-fast-math)"""
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(_SRC, [os.path.join(_HERE, "g2o_restated.h")], (*flags, "-D_GNU_SOURCE")))
        vp = C.c_void_p
        L.s3x_set_ulp.argtypes = [C.c_uint64]; L.s3x_set_ulp.restype = None
        L.s3x_from_rts.argtypes = [vp, vp, C.c_float, vp]; L.s3x_from_rts.restype = None
        L.s3x_exp.argtypes = [vp, vp]; L.s3x_exp.restype = None
        L.s3x_mul.argtypes = [vp, vp, vp]; L.s3x_mul.restype = None
        L.s3x_inverse.argtypes = [vp, vp]; L.s3x_inverse.restype = None
        L.s3x_map.argtypes = [vp, vp, vp]; L.s3x_map.restype = None
        L.s3x_ldlt7.argtypes = [vp, vp, vp]; L.s3x_ldlt7.restype = C.c_int
        L.s3x_linearize.argtypes = [vp, C.c_int] + [vp] * 8; L.s3x_linearize.restype = None
        L.s3x_prepare.argtypes = [vp, vp, C.c_int, vp]; L.s3x_prepare.restype = None
        L.s3x_pair_chi2.argtypes = [vp] * 6 + [C.c_int] + [vp] * 4; L.s3x_pair_chi2.restype = None
        L.s3x_optimize.argtypes = [vp] * 6 + [C.c_int] + [vp] * 4 + [C.c_float, C.c_float, C.c_int] + [vp] * 5; L.s3x_optimize.restype = None
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sim3(q, t, s):
    return Sim3((C.c_double * 4)(*q), (C.c_double * 3)(*t), float(s))


def sim3_exp(u, ulp_seed=0):
    u = np.ascontiguousarray(u, np.float64); o = Sim3()
    lib().s3x_set_ulp(ulp_seed)
    lib().s3x_exp(_p(u), C.byref(o))
    lib().s3x_set_ulp(0)
    return o


def mul(a, b):
    o = Sim3(); lib().s3x_mul(C.byref(a), C.byref(b), C.byref(o)); return o


def inverse(a):
    o = Sim3(); lib().s3x_inverse(C.byref(a), C.byref(o)); return o


def sim3_map(a, X):
    X = np.ascontiguousarray(X, np.float64); o = np.zeros(3)
    lib().s3x_map(C.byref(a), _p(X), _p(o))
    return o


def from_rts(R, t, s):
    R = np.ascontiguousarray(R, np.float32); t = np.ascontiguousarray(t, np.float32); o = Sim3()
    lib().s3x_from_rts(_p(R), _p(t), float(np.float32(s)), C.byref(o))
    return o


def ldlt7(H, b):
    H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(7)
    ok = lib().s3x_ldlt7(_p(H), _p(b), _p(x))
    return bool(ok), x


def prepare(prob):
    """(P1c, P2c) [n, 3] float64: vPoint1 / vPoint2 of a problem dict (tests/sim3_opt_scenes.py)"""
    n = prob["n"]
    out = []
    for X, T in ((prob["X1w"], prob["Tcw1"]), (prob["X2w"], prob["Tcw2"])):
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 3); T = np.ascontiguousarray(T, np.float32); Xc = np.zeros((n, 3))
        lib().s3x_prepare(_p(X), _p(T), n, _p(Xc))
        out.append(Xc)
    return out


def _edges(prob, inv_sigma2):
    f = lambda k, d: np.ascontiguousarray(prob[k], d)
    sg = np.ascontiguousarray(inv_sigma2, np.float32)
    P1, P2 = prepare(prob)
    return (P1, P2, f("obs1", np.float32), f("obs2", np.float32), np.ascontiguousarray(sg[f("octave1", np.int64)]),
            np.ascontiguousarray(sg[f("octave2", np.int64)]))


def linearize(est, fix_scale, P1, P2, obs1, obs2, cam1, cam2):
    """(J12 [2, 7], J21 [2, 7]) of one pair: g2o's numeric linearizeOplus"""
    a = [np.ascontiguousarray(P1, np.float64), np.ascontiguousarray(P2, np.float64), np.ascontiguousarray(obs1, np.float32),
         np.ascontiguousarray(obs2, np.float32), np.ascontiguousarray(cam1, np.float32), np.ascontiguousarray(cam2, np.float32)]
    J12, J21 = np.zeros((2, 7)), np.zeros((2, 7))
    lib().s3x_linearize(C.byref(est), int(fix_scale), *[_p(x) for x in a], _p(J12), _p(J21))
    return J12, J21


def pair_chi2(prob, inv_sigma2, S):
    """[n, 2] chi2 of e12 / e21 of every pair at the Sim3 S"""
    P1, P2, o1, o2, i1, i2 = _edges(prob, inv_sigma2)
    out = np.zeros((prob["n"], 2))
    lib().s3x_pair_chi2(_p(P1), _p(P2), _p(o1), _p(o2), _p(i1), _p(i2), prob["n"], _p(np.ascontiguousarray(prob["cam1"], np.float32)),
                        _p(np.ascontiguousarray(prob["cam2"], np.float32)), C.byref(S), _p(out))
    return out


def optimize(prob, inv_sigma2, ulp_seed=0, flags=("-O2",)):
    """OptimizeSim3 of a problem dict: dict(res Result, kept [n] bool, cut_chi [2, n, 2], est [3] Sim3 (initial, after round 1, last
    tried), trace Trace)"""
    n = prob["n"]
    P1, P2, o1, o2, i1, i2 = _edges(prob, inv_sigma2)
    cam1, cam2 = np.ascontiguousarray(prob["cam1"], np.float32), np.ascontiguousarray(prob["cam2"], np.float32)
    R, t = np.ascontiguousarray(prob["R12"], np.float32), np.ascontiguousarray(prob["t12"], np.float32)
    res, tr, est = Result(), Trace(), (Sim3 * 3)()
    kept = np.zeros(max(n, 1), np.uint8); cut = np.zeros((2, max(n, 1), 2))
    L = lib(flags)
    L.s3x_set_ulp(ulp_seed)
    L.s3x_optimize(_p(P1), _p(P2), _p(o1), _p(o2), _p(i1), _p(i2), n, _p(cam1), _p(cam2), _p(R), _p(t), float(np.float32(prob["s12"])),
                   float(np.float32(prob["th2"])), int(prob["fix_scale"]), C.byref(res), _p(kept), _p(cut), est, C.byref(tr))
    L.s3x_set_ulp(0)
    return dict(res=res, kept=kept[:n].astype(bool), cut_chi=cut[:, :n], est=list(est), trace=tr)
