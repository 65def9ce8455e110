"""Initializer (src/Initializer.cc) over orbm_init_find_models / orbm_init_reconstruct_f: the monocular initialisation with every
H / F hypothesis evaluated on the device in one launch, the folds of FindHomography / FindFundamental and ReconstructF's choice
among the four motions in the library, and CheckRT for up to 8 motions in one launch.

Two differences to the reference.  ReconstructH (:572-732) is not built: this fork takes it only at RH > 0.99 (:115), and
Initializer.initialize reports that case as WANTS_RECONSTRUCT_H.  When no F hypothesis scores above 0 the reference leaves
vbMatchesInliersF empty and F21 an empty cv::Mat and ReconstructF throws; here that is the status NO_FUNDAMENTAL."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr as _p


class InitModels(C.Structure):
    """orbm_init_models"""
    _fields_ = [("H21", C.c_float * 9), ("F21", C.c_float * 9), ("SH", C.c_float), ("SF", C.c_float), ("itH", C.c_int32), ("itF", C.c_int32)]


class InitReconstruction(C.Structure):
    """orbm_init_reconstruction"""
    _fields_ = [("R21", C.c_float * 9), ("t21", C.c_float * 3), ("parallax", C.c_float * 4), ("ngood", C.c_int32 * 4), ("found", C.c_int32),
                ("best", C.c_int32), ("N", C.c_int32), ("max_good", C.c_int32), ("nsimilar", C.c_int32)]


MAX_N, MAX_H, MAX_MOTIONS = 8192, 1024, 8
NOT_INITIALIZED, INITIALIZED, WANTS_RECONSTRUCT_H, NO_FUNDAMENTAL = 0, 1, 2, 3


def _f(a, dtype, shape):
    return np.ascontiguousarray(a, dtype).reshape(shape)


def unpack_mask(words, n):
    """[.., (n + 63) // 64] uint64 -> [.., n] bool: bit i % 64 of word i // 64"""
    w = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(*w.shape[:-1], -1), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def find_models(keys1, keys2, matches, sets, sigma=1.0, per_hypothesis=False):
    """orbm_init_find_models: FindHomography and FindFundamental over the pre-drawn sets [H][8] in one launch.  keys1 / keys2 =
    every undistorted keypoint position of the two frames, matches [n][2] = mvMatches12.  Returns a dict: H21, F21 [3, 3], SH, SF,
    itH, itF (-1: no hypothesis scored above 0), inliersH, inliersF [n] bool, maskH, maskF (the uint64 words); with
    per_hypothesis also matrices [2, H, 3, 3], scores [2, H], masks [2, H, words] (model 0 = H, 1 = F)."""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m, s = _f(matches, np.int32, (-1, 2)), _f(sets, np.int32, (-1, 8))
    n, H, words = len(m), len(s), (len(m) + 63) // 64
    out = InitModels()
    mh, mf = np.zeros(max(words, 1), np.uint64), np.zeros(max(words, 1), np.uint64)
    hm = hs = hk = None
    if per_hypothesis:
        hm, hs, hk = np.zeros((2, max(H, 1), 9), np.float32), np.zeros((2, max(H, 1)), np.float32), np.zeros((2, max(H, 1), max(words, 1)), np.uint64)
    check(lib().orbm_init_find_models(_p(k1), len(k1), _p(k2), len(k2), _p(m), n, _p(s), H, float(sigma), C.byref(out), _p(mh), _p(mf),
                                      None if hm is None else _p(hm), None if hs is None else _p(hs), None if hk is None else _p(hk)))
    res = dict(H21=np.array(out.H21, np.float32).reshape(3, 3), F21=np.array(out.F21, np.float32).reshape(3, 3), SH=np.float32(out.SH),
               SF=np.float32(out.SF), itH=out.itH, itF=out.itF, maskH=mh[:words], maskF=mf[:words],
               inliersH=unpack_mask(mh[:words], n), inliersF=unpack_mask(mf[:words], n))
    if per_hypothesis:
        res.update(matrices=hm[:, :H].reshape(2, H, 3, 3), scores=hs[:, :H], masks=hk[:, :H, :words])
    return res


def check_rt(keys1, keys2, matches, inliers, K, R, t, th2):
    """orbm_init_check_rt: CheckRT of M <= 8 motions (R [M, 3, 3], t [M, 3]) in one launch.  Returns a dict: ngood [M], parallax [M],
    good [M, n1] bool, P3D [M, n1, 3], counted [M, n] bool, cos_parallax [M, n]."""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m = _f(matches, np.int32, (-1, 2))
    inl = _f(np.asarray(inliers).astype(np.uint8), np.uint8, (-1,))
    Kf, Rf, tf = _f(K, np.float32, (9,)), _f(R, np.float32, (-1, 9)), _f(t, np.float32, (-1, 3))
    n, n1, M = len(m), len(k1), len(Rf)
    if len(inl) != n or len(tf) != M:
        raise ValueError("inliers / t differ in length from matches / R")
    good, P3D = np.zeros((max(M, 1), max(n1, 1)), np.uint8), np.zeros((max(M, 1), max(n1, 1), 3), np.float32)
    counted, cosp = np.zeros((max(M, 1), max(n, 1)), np.uint8), np.zeros((max(M, 1), max(n, 1)), np.float32)
    ngood, parallax = np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.float32)
    check(lib().orbm_init_check_rt(_p(k1), n1, _p(k2), len(k2), _p(m), n, _p(inl), _p(Kf), _p(Rf), _p(tf), M, float(np.float32(th2)), _p(good),
                                   _p(P3D), _p(counted), _p(cosp), _p(ngood), _p(parallax)))
    if n1 == 0 or n == 0:           # the arrays above were padded to one entry
        good, P3D, counted, cosp = good[:, :n1], P3D[:, :n1], counted[:, :n], cosp[:, :n]
    return dict(ngood=ngood[:M], parallax=parallax[:M], good=good[:M].astype(bool), P3D=P3D[:M], counted=counted[:M].astype(bool),
                cos_parallax=cosp[:M])


def reconstruct_f(keys1, keys2, matches, inliers, F21, K, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    """orbm_init_reconstruct_f: ReconstructF.  Returns a dict: found, R21 [3, 3], t21 [3], P3D [n1, 3], triangulated [n1] bool, ngood [4],
    parallax [4], best, N."""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m = _f(matches, np.int32, (-1, 2))
    inl = _f(np.asarray(inliers).astype(np.uint8), np.uint8, (-1,))
    if len(inl) != len(m):
        raise ValueError("inliers differ in length from matches")
    Ff, Kf = _f(F21, np.float32, (9,)), _f(K, np.float32, (9,))
    n1 = len(k1)
    out = InitReconstruction()
    P3D, tri = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    check(lib().orbm_init_reconstruct_f(_p(k1), n1, _p(k2), len(k2), _p(m), len(m), _p(inl), _p(Ff), _p(Kf), float(sigma), float(min_parallax),
                                        int(min_triangulated), C.byref(out), _p(P3D), _p(tri)))
    return dict(found=bool(out.found), R21=np.array(out.R21, np.float32).reshape(3, 3), t21=np.array(out.t21, np.float32), P3D=P3D[:n1],
                triangulated=tri[:n1].astype(bool), ngood=np.array(out.ngood), parallax=np.array(out.parallax, np.float32), best=out.best, N=out.N)


def last_init_waits():
    """orbm_debug_last_init_waits: host waits of the last orbm_init_* call of this process."""
    return lib().orbm_debug_last_init_waits()


def debug_svd(shape, A):
    """orbm_debug_init_svd (test aid): shape 0 / 1 / 3 -> the last row of vt of a 16 x 9 / 8 x 9 / 4 x 4 matrix; 2 -> (w, u, vt) of a 3 x 3"""
    rows, cols = ((16, 9), (8, 9), (3, 3), (4, 4))[shape]
    A = _f(A, np.float32, (rows * cols,))
    w, u, vt = np.zeros(3, np.float32), np.zeros(9, np.float32), np.zeros(9, np.float32)
    check(lib().orbm_debug_init_svd(shape, _p(A), _p(w), _p(u), _p(vt)))
    return (w, u.reshape(3, 3), vt.reshape(3, 3)) if shape == 2 else vt[:cols].copy()


def draw_sets(n, H, randint):
    """the draw loop of :82-97 for H iterations; randint(lo, hi) is inclusive, as DUtils::Random::RandomInt"""
    out = np.zeros((H, 8), np.int32)
    for h in range(H):
        avail = list(range(n))
        for j in range(8):
            r = randint(0, len(avail) - 1)
            out[h, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Initializer:
    """The reference's Initializer: the constructor takes the reference frame's undistorted keypoint positions, K, sigma and the
    iteration count (Tracking.cc:732 builds it with sigma = 1.0, 200 iterations)."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200):
        if iterations > MAX_H:
            raise ValueError(f"more than {MAX_H} iterations")
        self.mvKeys1 = _f(keys1, np.float32, (-1, 2))
        self.mK = _f(K, np.float32, (3, 3))
        self.mSigma, self.mMaxIterations = float(sigma), int(iterations)
        self.mvMatches12 = self.mvSets = self.models = self.reconstruction = None
        self.RH = np.float32(np.nan)

    def initialize(self, keys2, matches12, draw=None, sets=None):
        """Initialize(CurrentFrame, vMatches12, ..): matches12 [n1] = index into keys2 or -1.  The sets come from `draw`, a callable
        (lo, hi) -> int drawn in the reference's order (:82-97), or pre-drawn as `sets` [iterations][8].  Returns (status, R21, t21,
        P3D [n1, 3], triangulated [n1] bool); status INITIALIZED, NOT_INITIALIZED, WANTS_RECONSTRUCT_H (RH > 0.99: the caller runs
        ReconstructH on self.models' H21 and inliersH) or NO_FUNDAMENTAL."""
        if (draw is None) == (sets is None):
            raise ValueError("give either draw or sets")
        keys2 = _f(keys2, np.float32, (-1, 2))
        v = np.asarray(matches12, np.int64).reshape(-1)
        if len(v) != len(self.mvKeys1):
            raise ValueError("matches12 must have one entry per reference keypoint")
        first = np.nonzero(v >= 0)[0]
        self.mvMatches12 = np.stack([first, v[first]], 1).astype(np.int32)
        n, n1 = len(first), len(self.mvKeys1)
        H = self.mMaxIterations
        self.mvSets = draw_sets(n, H, draw) if draw is not None else _f(sets, np.int32, (-1, 8))[:H]
        if len(self.mvSets) < H:
            raise ValueError("fewer pre-drawn sets than iterations")
        none = (np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((n1, 3), np.float32), np.zeros(n1, bool))
        self.reconstruction = None
        self.models = find_models(self.mvKeys1, keys2, self.mvMatches12, self.mvSets, self.mSigma)
        SH, SF = self.models["SH"], self.models["SF"]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.RH = np.float32(SH) / (np.float32(SH) + np.float32(SF))
        if float(self.RH) > 0.99:                   # a float against the double 0.99, as :115 compares
            return (WANTS_RECONSTRUCT_H,) + none
        if self.models["itF"] < 0:
            return (NO_FUNDAMENTAL,) + none
        r = reconstruct_f(self.mvKeys1, keys2, self.mvMatches12, self.models["inliersF"], self.models["F21"], self.mK, self.mSigma, 0.95, 60)
        self.reconstruction = r
        return (INITIALIZED if r["found"] else NOT_INITIALIZED, r["R21"], r["t21"], r["P3D"], r["triangulated"])
