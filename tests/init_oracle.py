"""ctypes wrapper of tests/init_oracle.c, the CPU restatement of the monocular Initializer (src/Initializer.cc): the general
cv::SVDecomp routine with its RNG tail, Normalize, ComputeH21 / ComputeF21, CheckHomography / CheckFundamental, the two folds,
CheckRT, DecomposeE, ReconstructF and Initialize (test infrastructure: never part of the product).  The C file is compiled on
first use into a per-user cache directory (tests/c_oracle.py).

No OpenCV exists for this project to run, so the restated cv::SVDecomp, cv::invert and cv::Mat products are unpinned like the other
OpenCV primitives (DESIGN sections 5 and 19); tests/test_cpu_init.py checks them from first principles against numpy in float64."""
import ctypes as C
import os

import numpy as np

import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "init_oracle.c")
_LIBS = {}

TH_H, TH_F = np.float32(5.991), np.float32(3.841)     # the chiSquare thresholds of CheckHomography / CheckFundamental


def lib(flags=("-O2",)):
    """the restatement built with `flags` (always -ffp-contract=off -fno-fast-math)"""
    if flags not in _LIBS:
        L = C.CDLL(c_oracle.build(_SRC, flags=flags))
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.io_rng_outputs.argtypes = [C.c_uint64, i, vp]; L.io_rng_outputs.restype = None
        L.io_svdecomp.argtypes = [vp, i, i, i, vp, vp, vp]; L.io_svdecomp.restype = i
        L.io_svd_vt3.argtypes = [vp, vp]; L.io_svd_vt3.restype = i
        L.io_invert33.argtypes = [vp, vp]; L.io_invert33.restype = None
        L.io_normalize.argtypes = [vp, i, vp, vp]; L.io_normalize.restype = None
        L.io_compute_h21.argtypes = [vp, vp, vp]; L.io_compute_h21.restype = None
        L.io_compute_f21.argtypes = [vp, vp, vp]; L.io_compute_f21.restype = None
        L.io_find_model.argtypes = [i, vp, i, vp, i, vp, i, vp, i, f] + [vp] * 8; L.io_find_model.restype = None
        L.io_check_rt.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp, vp, f, vp, vp, vp, vp, vp]; L.io_check_rt.restype = i
        L.io_decompose_e.argtypes = [vp] * 4; L.io_decompose_e.restype = None
        L.io_reconstruct_f.argtypes = [vp, vp, vp, vp, i, vp, vp, i, f, f, i] + [vp] * 7; L.io_reconstruct_f.restype = i
        L.io_initialize.argtypes = [vp, i, vp, i, vp, vp, i, f, vp] + [vp] * 7; L.io_initialize.restype = i
        _LIBS[flags] = L
    return _LIBS[flags]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, dtype, shape):
    return np.ascontiguousarray(a, dtype).reshape(shape)


def rng_outputs(seed, count):
    out = np.zeros(count, np.uint32)
    lib().io_rng_outputs(seed, count, _p(out))
    return out


def svdecomp(A, full_uv=True):
    """(w, u, vt, sweeps) of the restated cv::SVDecomp(A, w, u, vt, FULL_UV or 0) of a float matrix"""
    A = np.ascontiguousarray(A, np.float32)
    rows, cols = A.shape
    big, small = max(rows, cols), min(rows, cols)
    urows = big if full_uv else small
    w = np.zeros(small, np.float32)
    u = np.zeros((rows, urows) if rows >= cols else (rows, rows), np.float32)
    vt = np.zeros((cols, cols) if rows >= cols else (urows, cols), np.float32)
    sweeps = lib().io_svdecomp(_p(A), rows, cols, int(full_uv), _p(w), _p(u), _p(vt))
    return w, u, vt, sweeps


def svd_vt3(A):
    A = _f(A, np.float32, (16,)); v = np.zeros(4, np.float32)
    lib().io_svd_vt3(_p(A), _p(v))
    return v


def invert33(S):
    S = _f(S, np.float32, (9,)); D = np.zeros((3, 3), np.float32)
    lib().io_invert33(_p(S), _p(D))
    return D


def normalize(keys):
    k = _f(keys, np.float32, (-1, 2)); pn = np.zeros_like(k); T = np.zeros((3, 3), np.float32)
    lib().io_normalize(_p(k), len(k), _p(pn), _p(T))
    return pn, T


def compute_h21(p1, p2):
    a, b, H = _f(p1, np.float32, (8, 2)), _f(p2, np.float32, (8, 2)), np.zeros((3, 3), np.float32)
    lib().io_compute_h21(_p(a), _p(b), _p(H))
    return H


def compute_f21(p1, p2):
    a, b, F = _f(p1, np.float32, (8, 2)), _f(p2, np.float32, (8, 2)), np.zeros((3, 3), np.float32)
    lib().io_compute_f21(_p(a), _p(b), _p(F))
    return F


def find_model(model, keys1, keys2, matches, sets, sigma=1.0, flags=("-O2",)):
    """FindHomography (model 0) / FindFundamental (1): dict(matrices [H, 3, 3], scores [H], flags [H, n] bool, chi [H, n, 2], M [3, 3],
    S, inliers [n] bool, it)"""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m, s = _f(matches, np.int32, (-1, 2)), _f(sets, np.int32, (-1, 8))
    n, H = len(m), len(s)
    mats, scores = np.zeros((max(H, 1), 3, 3), np.float32), np.zeros(max(H, 1), np.float32)
    fl, chi = np.zeros((max(H, 1), max(n, 1)), np.uint8), np.zeros((max(H, 1), max(n, 1), 2), np.float32)
    if n:
        fl, chi = np.zeros((max(H, 1), n), np.uint8), np.zeros((max(H, 1), n, 2), np.float32)
    M, S, inl, it = np.zeros((3, 3), np.float32), np.zeros(1, np.float32), np.zeros(max(n, 1), np.uint8), np.zeros(1, np.int32)
    lib(flags).io_find_model(model, _p(k1), len(k1), _p(k2), len(k2), _p(m), n, _p(s), H, float(sigma), _p(mats), _p(scores), _p(fl), _p(chi), _p(M),
                             _p(S), _p(inl), _p(it))
    return dict(matrices=mats[:H], scores=scores[:H], flags=fl[:H, :n].astype(bool), chi=chi[:H, :n], M=M, S=S[0], inliers=inl[:n].astype(bool),
                it=int(it[0]))


def find_models(keys1, keys2, matches, sets, sigma=1.0):
    """both models, in the shape of orb_slam2_e_amd.find_models(per_hypothesis=True) plus chi [2, H, n, 2]"""
    h, f = (find_model(k, keys1, keys2, matches, sets, sigma) for k in (0, 1))
    return dict(H21=h["M"], F21=f["M"], SH=h["S"], SF=f["S"], itH=h["it"], itF=f["it"], inliersH=h["inliers"], inliersF=f["inliers"],
                matrices=np.stack([h["matrices"], f["matrices"]]), scores=np.stack([h["scores"], f["scores"]]),
                flags=np.stack([h["flags"], f["flags"]]), chi=np.stack([h["chi"], f["chi"]]))


def check_rt(keys1, keys2, matches, inliers, K, R, t, th2):
    """CheckRT of one motion: dict(ngood, parallax, good [n1] bool, P3D [n1, 3], counted [n] bool, cos_parallax [n], err [n, 2])"""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m = _f(matches, np.int32, (-1, 2))
    inl = _f(np.asarray(inliers).astype(np.uint8), np.uint8, (-1,))
    Kf, Rf, tf = _f(K, np.float32, (9,)), _f(R, np.float32, (9,)), _f(t, np.float32, (3,))
    n, n1 = len(m), len(k1)
    good, P3D = np.zeros(max(n1, 1), np.uint8), np.zeros((max(n1, 1), 3), np.float32)
    counted, cosp, err = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 2), np.float32)
    par = np.zeros(1, np.float32)
    ng = lib().io_check_rt(_p(Rf), _p(tf), _p(k1), n1, _p(k2), _p(m), n, _p(inl), _p(Kf), _p(P3D), float(np.float32(th2)), _p(good), _p(par),
                           _p(counted), _p(cosp), _p(err))
    return dict(ngood=ng, parallax=par[0], good=good[:n1].astype(bool), P3D=P3D[:n1], counted=counted[:n].astype(bool), cos_parallax=cosp[:n],
                err=err[:n])


def decompose_e(E):
    E = _f(E, np.float32, (9,)); R1, R2, t = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    lib().io_decompose_e(_p(E), _p(R1), _p(R2), _p(t))
    return R1, R2, t


def reconstruct_f(keys1, keys2, matches, inliers, F21, K, sigma=1.0, min_parallax=1.0, min_triangulated=50, flags=("-O2",)):
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    m = _f(matches, np.int32, (-1, 2))
    inl = _f(np.asarray(inliers).astype(np.uint8), np.uint8, (-1,))
    Ff, Kf = _f(F21, np.float32, (9,)), _f(K, np.float32, (9,))
    n1 = len(k1)
    R21, t21, P3D, tri = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    ngood, par, best = np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(1, np.int32)
    found = lib(flags).io_reconstruct_f(_p(inl), _p(Ff), _p(Kf), _p(k1), n1, _p(k2), _p(m), len(m), float(sigma), float(min_parallax), int(min_triangulated),
                                   _p(R21), _p(t21), _p(P3D), _p(tri), _p(ngood), _p(par), _p(best))
    return dict(found=bool(found), R21=R21, t21=t21, P3D=P3D[:n1], triangulated=tri[:n1].astype(bool), ngood=ngood, parallax=par, best=int(best[0]))


def initialize(keys1, keys2, matches12, sets, K, sigma=1.0):
    """Initialize: dict(status 0 not initialised / 1 initialised / 2 RH > 0.99 / 3 no fundamental matrix, RH, R21, t21, P3D,
    triangulated, matches [n, 2])"""
    k1, k2 = _f(keys1, np.float32, (-1, 2)), _f(keys2, np.float32, (-1, 2))
    v, s, Kf = _f(matches12, np.int32, (-1,)), _f(sets, np.int32, (-1, 8)), _f(K, np.float32, (9,))
    n1 = len(k1)
    mo, no, RH = np.zeros((max(n1, 1), 2), np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    R21, t21, P3D, tri = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    st = lib().io_initialize(_p(k1), n1, _p(k2), len(k2), _p(v), _p(s), len(s), float(sigma), _p(Kf), _p(mo), _p(no), _p(RH), _p(R21), _p(t21),
                             _p(P3D), _p(tri))
    return dict(status=st, RH=RH[0], R21=R21, t21=t21, P3D=P3D[:n1], triangulated=tri[:n1].astype(bool), matches=mo[:no[0]])


def masks_of(flags):
    """[.., n] bool -> [.., (n + 63) // 64] uint64, bit i % 64 of word i // 64"""
    flags = np.asarray(flags)
    n = flags.shape[-1]
    W = (n + 63) // 64
    padded = np.zeros(flags.shape[:-1] + (W * 64,), np.uint8); padded[..., :n] = flags
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(flags.shape[:-1] + (W,))
