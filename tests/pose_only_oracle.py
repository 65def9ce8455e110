"""ctypes wrapper of tests/pose_only_oracle.c, the CPU restatement of Optimizer::PoseOptimization (test infrastructure: never part
of the product).  The C file is compiled on first use into a per-user cache directory (tests/c_oracle.py)."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "pose_only_oracle.c")
_LIB = None


class Stats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4), ("ninitial", C.c_int32),
                ("chi2", C.c_double), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("min_rho", C.c_double), ("min_class", C.c_double), ("min_stop", C.c_double), ("round_chi2", C.c_double * 4),
                ("chi2_plain", C.c_double * 4), ("chi2_robust", C.c_double * 4)]


class SE3(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3)]


class Cam(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double)]


EDGE_DTYPE = np.dtype([("obs", "f8", 3), ("Xw", "f8", 3), ("info", "f8"), ("stereo", "i4"), ("kp", "i4"), ("level", "i4"),
                       ("robust", "i4"), ("err", "f8", 3), ("level_r4", "i4"), ("pad", "i4")])     # po_edge
EDGE_BYTES = EDGE_DTYPE.itemsize


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(c_oracle.build(_SRC, [os.path.join(_HERE, "g2o_restated.h")]))
        vp = C.c_void_p
        L.po_pose_optimization.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats), vp]
        L.po_pose_optimization.restype = C.c_int
        L.po_ldlt_solve.argtypes = [vp, vp, C.c_int, vp]
        L.po_ldlt_solve.restype = C.c_int
        L.po_exp.argtypes = [vp, C.POINTER(SE3)]
        L.po_compose.argtypes = [C.POINTER(SE3), C.POINTER(SE3), C.POINTER(SE3)]
        L.po_from_cv.argtypes = [vp, C.POINTER(SE3)]
        L.po_to_cv.argtypes = [C.POINTER(SE3), vp]
        L.po_quat_from_matrix.argtypes = [vp, vp]
        L.po_quat_to_matrix.argtypes = [vp, vp]
        L.po_edge_error.argtypes = [C.POINTER(Cam), C.c_int, vp, vp, C.POINTER(SE3), vp]
        L.po_edge_jacobian.argtypes = [C.POINTER(Cam), C.c_int, vp, C.POINTER(SE3), vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pose_optimization(kp_xy, octave, uright, has_mp, mp_pos, cam, inv_sigma2, Tcw, outlier_in=None, edges=False):
    """Optimizer::PoseOptimization on flat frame arrays.  cam = (fx, fy, cx, cy, mbf).  Returns
    (ngood, Tcw_out float32[4, 4], outlier uint8[n] (outlier_in, or 0, where has_mp is not set), Stats), and with edges=True
    also the graph's edges (EDGE_DTYPE, one per keypoint with a map point, in keypoint order) as the call left them."""
    n = len(has_mp)
    kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(n, 2)
    octave = np.ascontiguousarray(octave, np.int32)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
    has_mp = np.ascontiguousarray(has_mp, np.uint8)
    mp_pos = np.ascontiguousarray(mp_pos, np.float32).reshape(n, 3)
    camv = np.ascontiguousarray(cam, np.float32)
    inv = np.ascontiguousarray(inv_sigma2, np.float32)
    Tin = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
    Tout = np.zeros((4, 4), np.float32)
    outlier = np.zeros(n, np.uint8) if outlier_in is None else np.array(outlier_in, np.uint8)
    st = Stats()
    scratch = np.zeros(max(n, 1) * EDGE_BYTES, np.uint8)
    ng = lib().po_pose_optimization(_p(kp_xy), _p(octave), None if ur is None else _p(ur), n, _p(has_mp), _p(mp_pos), _p(camv), _p(inv),
                                    _p(Tin), _p(Tout), _p(outlier), C.byref(st), _p(scratch))
    if edges:
        return ng, Tout, outlier, st, scratch[:int(has_mp.sum()) * EDGE_BYTES].view(EDGE_DTYPE).copy()
    return ng, Tout, outlier, st


def ldlt_solve(A, b):
    """Eigen LDLT as LinearSolverDense uses it: x, or None where isPositive() is false."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(len(b))
    ok = lib().po_ldlt_solve(_p(A), _p(b), len(b), _p(x))
    return x if ok else None


def se3(q, t):
    s = SE3()
    s.q[:] = [float(v) for v in q]
    s.t[:] = [float(v) for v in t]
    return s


def se3_exp(u):
    s = SE3()
    lib().po_exp(_p(np.ascontiguousarray(u, np.float64)), C.byref(s))
    return s


def se3_compose(a, b):
    s = SE3()
    lib().po_compose(C.byref(a), C.byref(b), C.byref(s))
    return s


def se3_from_cv(T):
    s = SE3()
    lib().po_from_cv(_p(np.ascontiguousarray(T, np.float32).reshape(16)), C.byref(s))
    return s


def se3_to_cv(s):
    T = np.zeros(16, np.float32)
    lib().po_to_cv(C.byref(s), _p(T))
    return T.reshape(4, 4)


def quat_from_matrix(R):
    q = np.zeros(4)
    lib().po_quat_from_matrix(_p(np.ascontiguousarray(R, np.float64).reshape(9)), _p(q))
    return q


def quat_to_matrix(q):
    R = np.zeros(9)
    lib().po_quat_to_matrix(_p(np.ascontiguousarray(q, np.float64)), _p(R))
    return R.reshape(3, 3)


def cam_struct(cam):
    c = Cam()
    c.fx, c.fy, c.cx, c.cy, c.bf = [float(np.float32(v)) for v in cam]
    return c


def edge_error(cam, stereo, obs, Xw, T):
    e = np.zeros(3)
    lib().po_edge_error(C.byref(cam_struct(cam)), int(stereo), _p(np.ascontiguousarray(obs, np.float64)),
                        _p(np.ascontiguousarray(Xw, np.float64)), C.byref(T), _p(e))
    return e if stereo else e[:2]


def edge_jacobian(cam, stereo, Xw, T):
    J = np.zeros(18)
    lib().po_edge_jacobian(C.byref(cam_struct(cam)), int(stereo), _p(np.ascontiguousarray(Xw, np.float64)), C.byref(T), _p(J))
    return J.reshape(3, 6)[:3 if stereo else 2]


def run(p, **kw):
    """pose_optimization on a tests/pose_only_scene.py problem dict"""
    return pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"], p["Tcw"], **kw)
