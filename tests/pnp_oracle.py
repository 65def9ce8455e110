"""ctypes wrapper of tests/pnp_oracle.c, the literal CPU restatement of PnPsolver (src/PnPsolver.cc): EPnP, CheckInliers, Refine,
SetRansacParameters and the folds of both iterate functions (test infrastructure: never part of the product).  The C file is
compiled on first use into a per-user cache directory (tests/c_oracle.py).

No OpenCV exists for this project to run, so the restated cvSVD / cvInvert / cvSolve / cvMulTransposed are unpinned like the other
OpenCV primitives; tests/test_cpu_pnp.py checks them from first principles against numpy in float64.
LIBM = the build whose SVD calls libm's hypot, as the reference's does (-DPNP_LIBM_HYPOT)."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "pnp_oracle.c")
_LIBS = {}
DEFAULT, LIBM = ("-O2",), ("-O2", "-DPNP_LIBM_HYPOT")


class Fold(C.Structure):        # pno_fold
    _fields_ = [("N", C.c_int32), ("min_inliers", C.c_int32), ("max_its", C.c_int32), ("iterations", C.c_int32), ("best_inliers", C.c_int32),
                ("best", C.c_int32), ("epsilon", C.c_float), ("last_refined", C.c_int32)]


def lib(flags=DEFAULT):
    """the restatement built with `flags` (always -ffp-contract=off -fno-fast-math)"""
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(_SRC, flags=flags))
        vp, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
        L.pno_solve_svd.argtypes = [vp, i, i, vp, vp]; L.pno_solve_svd.restype = None
        L.pno_invert_svd.argtypes = [vp, i, vp]; L.pno_invert_svd.restype = None
        L.pno_svd_ut.argtypes = [vp, i, vp, vp]; L.pno_svd_ut.restype = None
        L.pno_pose.argtypes = [vp, vp, i, vp, vp, vp, vp]; L.pno_pose.restype = i
        L.pno_check_inliers.argtypes = [vp, vp, vp, vp, vp, i, vp, vp]; L.pno_check_inliers.restype = i
        L.pno_refine.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp]; L.pno_refine.restype = i
        L.pno_problem.argtypes = [vp, vp, vp, vp, i, i, vp, f, vp, i, i] + [vp] * 11; L.pno_problem.restype = None
        L.pno_set_ransac_parameters.argtypes = [vp, d, i, i, i, f]; L.pno_set_ransac_parameters.restype = None
        L.pno_iterate.argtypes = [vp, vp, vp, i, i, vp, vp, vp]; L.pno_iterate.restype = i
        L.pno_iterate_frame_stage1.argtypes = [vp, vp, vp, vp, i, i, vp, vp]; L.pno_iterate_frame_stage1.restype = i
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def svd_ut(A, flags=DEFAULT):
    """cvSVD(A, W, Ut, 0, MODIFY_A | U_T) of a square matrix -> (W [n], Ut [n, n])"""
    A = np.ascontiguousarray(A, np.float64); n = len(A)
    W, Ut = np.zeros(n), np.zeros((n, n))
    lib(flags).pno_svd_ut(_p(A), n, _p(W), _p(Ut))
    return W, Ut


def solve_svd(A, b):
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(A.shape[1])
    lib().pno_solve_svd(_p(A), A.shape[0], A.shape[1], _p(b), _p(x))
    return x


def invert_svd(A):
    A = np.ascontiguousarray(A, np.float64); inv = np.zeros_like(A)
    lib().pno_invert_svd(_p(A), len(A), _p(inv))
    return inv


def pose(pws, us, cam, flags=DEFAULT):
    """compute_pose of correspondences in double -> (R [3, 3], t [3], rep_error, qr_solve early returns)"""
    pws = np.ascontiguousarray(pws, np.float64).reshape(-1, 3); us = np.ascontiguousarray(us, np.float64).reshape(-1, 2)
    cam = np.ascontiguousarray(cam, np.float64)
    R, t, rep = np.zeros((3, 3)), np.zeros(3), np.zeros(1)
    sing = lib(flags).pno_pose(_p(pws), _p(us), len(pws), _p(cam), _p(R), _p(t), _p(rep))
    return R, t, float(rep[0]), sing


def max_error(prob, sigma2):
    return (np.asarray(sigma2, np.float32)[np.asarray(prob["octave"])] * np.float32(prob["th2"])).astype(np.float32)


def check_inliers(R, t, prob, sigma2):
    """(flags [n] bool, count) of CheckInliers with the pose R, t"""
    R = np.ascontiguousarray(R, np.float64); t = np.ascontiguousarray(t, np.float64)
    X, uv, me = np.ascontiguousarray(prob["Xw"], np.float32), np.ascontiguousarray(prob["uv"], np.float32), max_error(prob, sigma2)
    cam = np.ascontiguousarray(prob["cam"], np.float64); flags = np.zeros(prob["n"], np.uint8)
    cnt = lib().pno_check_inliers(_p(R), _p(t), _p(X), _p(uv), _p(me), prob["n"], _p(cam), _p(flags))
    return flags.astype(bool), cnt


def refine(prob, sigma2, best, flags=DEFAULT):
    """Refine on the flags `best` -> (R, t, refined flags, mnRefinedInliers)"""
    X, uv, me = np.ascontiguousarray(prob["Xw"], np.float32), np.ascontiguousarray(prob["uv"], np.float32), max_error(prob, sigma2)
    cam = np.ascontiguousarray(prob["cam"], np.float64); b = np.ascontiguousarray(best, np.uint8)
    R, t, out = np.zeros((3, 3)), np.zeros(3), np.zeros(prob["n"], np.uint8)
    cnt = lib(flags).pno_refine(_p(X), _p(uv), _p(me), prob["n"], _p(cam), _p(b), _p(R), _p(t), _p(out))
    return R, t, out.astype(bool), cnt


def hypotheses(prob, sigma2, best_in=0, flags=DEFAULT):
    """what orbm_pnp_hypotheses returns for one problem: dict(R [H, 9], t [H, 3], rep_error [H], ninliers, refined, Rr, tr, nrefined,
    flags [H, n] bool, rflags [H, n] bool, singular [H])"""
    n, H = prob["n"], prob["H"]
    X, uv = np.ascontiguousarray(prob["Xw"], np.float32), np.ascontiguousarray(prob["uv"], np.float32)
    octave, sets = np.ascontiguousarray(prob["octave"], np.int32), np.ascontiguousarray(prob["sets"], np.int32).reshape(H, 4)
    cam, sg = np.ascontiguousarray(prob["cam"], np.float64), np.ascontiguousarray(sigma2, np.float32)
    o = dict(R=np.zeros((H, 9)), t=np.zeros((H, 3)), rep_error=np.zeros(H), ninliers=np.zeros(H, np.int32), refined=np.zeros(H, np.int32),
             Rr=np.zeros((H, 9)), tr=np.zeros((H, 3)), nrefined=np.zeros(H, np.int32), flags=np.zeros((H, n), np.uint8),
             rflags=np.zeros((H, n), np.uint8), singular=np.zeros(H, np.int32))
    lib(flags).pno_problem(_p(X), _p(uv), _p(octave), _p(sets), n, H, _p(cam), float(np.float32(prob["th2"])), _p(sg), prob["min_inliers"], best_in,
                           _p(o["R"]), _p(o["t"]), _p(o["rep_error"]), _p(o["ninliers"]), _p(o["refined"]), _p(o["Rr"]), _p(o["tr"]),
                           _p(o["nrefined"]), _p(o["flags"]), _p(o["rflags"]), _p(o["singular"]))
    o["flags"] = o["flags"].astype(bool); o["rflags"] = o["rflags"].astype(bool)
    return o


def masks_of(flags):
    """[H, n] bool -> [H, (n + 63) // 64] uint64, bit i % 64 of word i // 64"""
    H, n = flags.shape
    W = (n + 63) // 64
    padded = np.zeros((H, W * 64), np.uint8); padded[:, :n] = flags
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(H, W)


def ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
    """(mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)"""
    f = Fold(N, 0, 0, 0, 0, -1, 0.0, 0)
    lib().pno_set_ransac_parameters(C.byref(f), probability, minInliers, maxIterations, minSet, epsilon)
    return f.min_inliers, f.max_its, f.epsilon


def tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3).astype(np.float32); T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


class Solver:
    """PnPsolver over the restatement.  prob["sets"] are consumed in order; every iterate evaluates the hypotheses it may need
    with the carried best, as the reference's loop would."""

    def __init__(self, prob, sigma2, probability=0.99, minInliers=8, maxIterations=300, epsilon=0.4, flags=DEFAULT):
        self.prob, self.sigma2, self.flags = dict(prob), sigma2, flags
        self.fold = Fold(prob["n"], 0, 0, 0, 0, -1, 0.0, 0)
        lib().pno_set_ransac_parameters(C.byref(self.fold), probability, minInliers, maxIterations, 4, epsilon)
        self.all_sets = np.asarray(prob["sets"], np.int32).reshape(-1, 4)
        self.best_flags = self.refined = None

    def iterate(self, n):
        """(Tcw or None, bNoMore, flags [N] bool or None, nInliers, hypothesis index or -1, kind)"""
        f = self.fold
        if f.N < f.min_inliers:
            return None, True, None, 0, -1, 0
        start = f.iterations
        stop = start + max(f.max_its - start, n, 0)
        p = dict(self.prob, sets=self.all_sets[start:stop], H=stop - start, min_inliers=f.min_inliers)
        hyp = hypotheses(p, self.sigma2, best_in=f.best_inliers, flags=self.flags)
        counts = np.zeros(stop, np.int32); nref = np.zeros(stop, np.int32)
        counts[start:] = hyp["ninliers"]; nref[start:] = hyp["nrefined"]
        no_more, nin, kind = C.c_int(0), C.c_int(0), C.c_int(0)
        before = f.best
        h = lib().pno_iterate(C.byref(f), _p(counts), _p(nref), stop, n, C.byref(no_more), C.byref(nin), C.byref(kind))
        assert h != -2
        if f.best != before:                                        # the best moved in this call: its data are in this evaluation
            k = f.best - start
            self.best_flags = hyp["flags"][k]; self.best_pose = (hyp["R"][k], hyp["t"][k])
            self.refined = (hyp["Rr"][k], hyp["tr"][k], hyp["rflags"][k])
        if kind.value == 1:
            return tcw(self.refined[0], self.refined[1]), bool(no_more.value), self.refined[2], nin.value, h, 1
        if kind.value == 2:
            return tcw(*self.best_pose), bool(no_more.value), self.best_flags, nin.value, h, 2
        return None, bool(no_more.value), None, 0, -1, 0

    def find(self):
        return self.iterate(self.fold.max_its)
