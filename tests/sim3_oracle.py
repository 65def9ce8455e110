"""ctypes wrapper of tests/sim3_oracle.c, the CPU restatement of Sim3Solver (src/Sim3Solver.cc): the constructor's data
preparation, ComputeSim3, CheckInliers, SetRansacParameters and the fold of iterate (test infrastructure: never part of the product).
The C file is compiled on first use into a per-user cache directory (tests/c_oracle.py).

No OpenCV exists for this project to run, so the restated cv::eigen (JacobiImpl_<float>) and cv::Rodrigues are unpinned like the
other OpenCV primitives; tests/test_cpu_sim3.py checks them from first principles against numpy in float64."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sim3_oracle.c")
_LIBS = {}


class Fold(C.Structure):        # s3o_fold
    _fields_ = [("N", C.c_int32), ("min_inliers", C.c_int32), ("max_its", C.c_int32), ("iterations", C.c_int32), ("best_inliers", C.c_int32),
                ("best", C.c_int32)]


def lib(flags=("-O2",)):
    """the restatement built with `flags` (always -ffp-contract=off -fno-fast-math)"""
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(_SRC, flags=flags))
        vp = C.c_void_p
        L.s3o_eigen4.argtypes = [vp, vp, vp]; L.s3o_eigen4.restype = C.c_int
        L.s3o_rodrigues.argtypes = [vp, vp]; L.s3o_rodrigues.restype = None
        L.s3o_max_error.argtypes = [C.c_float]; L.s3o_max_error.restype = C.c_uint64
        L.s3o_is_inlier.argtypes = [C.c_float, C.c_float, C.c_uint64, C.c_uint64]; L.s3o_is_inlier.restype = C.c_int
        L.s3o_prepare.argtypes = [vp] * 9 + [C.c_int] + [vp] * 6; L.s3o_prepare.restype = None
        L.s3o_compute_sim3.argtypes = [vp, vp, C.c_int] + [vp] * 6; L.s3o_compute_sim3.restype = None
        L.s3o_hypotheses.argtypes = [vp] * 8 + [C.c_int, vp, C.c_int, C.c_int] + [vp] * 8; L.s3o_hypotheses.restype = None
        L.s3o_ransac_max_its.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int]; L.s3o_ransac_max_its.restype = C.c_int
        L.s3o_iterate.argtypes = [vp, vp, C.c_int, vp, vp]; L.s3o_iterate.restype = C.c_int
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def eigen4(N):
    """(eval [4] descending, evec [4, 4] rows, rotations) of the restated cv::eigen of a 4 x 4 symmetric float matrix"""
    N = np.ascontiguousarray(N, np.float32).reshape(16); w = np.zeros(4, np.float32); v = np.zeros((4, 4), np.float32)
    return w, v, lib().s3o_eigen4(_p(N), _p(w), _p(v))


def rodrigues(vec):
    v = np.ascontiguousarray(vec, np.float32); R = np.zeros((3, 3), np.float32)
    lib().s3o_rodrigues(_p(v), _p(R))
    return R


def max_error(sigma2):
    return int(lib().s3o_max_error(float(np.float32(sigma2))))


def is_inlier(err1, err2, max1, max2):
    return bool(lib().s3o_is_inlier(float(np.float32(err1)), float(np.float32(err2)), max1, max2))


def compute_sim3(p1, p2, fix_scale=False):
    """ComputeSim3 of two sets of three camera-frame points ([3, 3], row = point): dict(T12, R12, t12, s12, T21, N)"""
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    T12 = np.zeros((4, 4), np.float32); R = np.zeros((3, 3), np.float32); t = np.zeros(3, np.float32); s = np.zeros(1, np.float32)
    T21 = np.zeros((4, 4), np.float32); N = np.zeros((4, 4), np.float32)
    lib().s3o_compute_sim3(_p(p1), _p(p2), int(fix_scale), _p(T12), _p(R), _p(t), _p(s), _p(T21), _p(N))
    return dict(T12=T12, R12=R, t12=t, s12=s[0], T21=T21, N=N)


def prepare(prob, sigma2):
    """the constructor's data (:54-109) of a problem dict (tests/sim3_scenes.py)"""
    n = prob["n"]
    f = lambda k, d: np.ascontiguousarray(prob[k], d)
    X1, X2, o1, o2 = f("X1w", np.float32), f("X2w", np.float32), f("octave1", np.int32), f("octave2", np.int32)
    T1, T2 = f("Tcw1", np.float32), f("Tcw2", np.float32)
    cam1, cam2, sg = f("cam1", np.float32), f("cam2", np.float32), np.ascontiguousarray(sigma2, np.float32)
    out = dict(Xc1=np.zeros((n, 3), np.float32), Xc2=np.zeros((n, 3), np.float32), P1=np.zeros((n, 2), np.float32), P2=np.zeros((n, 2), np.float32),
               max1=np.zeros(n, np.uint64), max2=np.zeros(n, np.uint64), cam1=cam1, cam2=cam2, n=n)
    lib().s3o_prepare(_p(X1), _p(X2), _p(o1), _p(o2), _p(T1), _p(T2), _p(cam1), _p(cam2), _p(sg), n, _p(out["Xc1"]), _p(out["Xc2"]),
                      _p(out["P1"]), _p(out["P2"]), _p(out["max1"]), _p(out["max2"]))
    return out


def hypotheses(prob, sigma2, flags=("-O2",)):
    """every hypothesis of a problem: dict(T12 [H, 16], R12 [H, 9], t12 [H, 3], s12 [H], ninliers [H], flags [H, n] bool,
    gap [H, n], err [H, n, 2])"""
    pre = prepare(prob, sigma2)
    n, H = prob["n"], prob["H"]
    tri = np.ascontiguousarray(prob["triples"], np.int32).reshape(H, 3)
    out = dict(T12=np.zeros((H, 16), np.float32), R12=np.zeros((H, 9), np.float32), t12=np.zeros((H, 3), np.float32), s12=np.zeros(H, np.float32),
               ninliers=np.zeros(H, np.int32), flags=np.zeros((H, n), np.uint8), gap=np.ones((H, n)), err=np.zeros((H, n, 2), np.float32))
    lib(flags).s3o_hypotheses(_p(pre["Xc1"]), _p(pre["Xc2"]), _p(pre["P1"]), _p(pre["P2"]), _p(pre["max1"]), _p(pre["max2"]), _p(pre["cam1"]),
                              _p(pre["cam2"]), n, _p(tri), H, int(prob["fix_scale"]), _p(out["T12"]), _p(out["R12"]), _p(out["t12"]), _p(out["s12"]),
                              _p(out["ninliers"]), _p(out["flags"]), _p(out["gap"]), _p(out["err"]))
    out["flags"] = out["flags"].astype(bool)
    out["pre"] = pre
    return out


def masks_of(flags):
    """[H, n] bool -> [H, (n + 63) // 64] uint64, bit i % 64 of word i // 64"""
    H, n = flags.shape
    W = (n + 63) // 64
    padded = np.zeros((H, W * 64), np.uint8); padded[:, :n] = flags
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(H, W)


def ransac_max_its(probability, min_inliers, max_iterations, N):
    return lib().s3o_ransac_max_its(probability, min_inliers, max_iterations, N)


def draw_triples(n, H, randint):
    """the draw loop of :163-177, H times: randint(lo, hi) inclusive, as DUtils::Random::RandomInt"""
    out = np.zeros((H, 3), np.int32)
    for h in range(H):
        avail = list(range(n))
        for i in range(3):
            r = randint(0, len(avail) - 1)
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Solver:
    """Sim3Solver over the restatement: counts come from hypotheses(), iterate is s3o_iterate"""

    def __init__(self, prob, sigma2, probability=0.99, min_inliers=6, max_iterations=300, randint=None):
        self.prob, self.sigma2, self.randint = dict(prob), sigma2, randint
        self.N = prob["n"]
        self.fold = Fold(self.N, 0, 0, 0, 0, -1)
        self.hyp = None
        self.SetRansacParameters(probability, min_inliers, max_iterations)

    def SetRansacParameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.fold.min_inliers = min_inliers
        self.fold.max_its = ransac_max_its(probability, min_inliers, max_iterations, self.N)
        self.fold.iterations = 0

    def _evaluate(self):
        H = self.fold.max_its
        if self.randint is not None:
            self.prob["triples"] = draw_triples(self.N, H, self.randint)
        self.prob["triples"] = np.asarray(self.prob["triples"], np.int32).reshape(-1, 3)[:H]
        self.prob["H"] = H
        self.hyp = hypotheses(self.prob, self.sigma2)

    def iterate(self, n):
        """(index of the returned hypothesis or -1, bNoMore, inlier flags [N] or None, nInliers)"""
        if self.hyp is None and self.N >= self.fold.min_inliers:
            self._evaluate()
        counts = self.hyp["ninliers"] if self.hyp is not None else np.zeros(1, np.int32)
        no_more, nin = C.c_int(0), C.c_int(0)
        h = lib().s3o_iterate(C.byref(self.fold), _p(counts), n, C.byref(no_more), C.byref(nin))
        return h, bool(no_more.value), (self.hyp["flags"][h] if h >= 0 else None), nin.value

    def find(self):
        return self.iterate(self.fold.max_its)
