"""PnPsolver on the device, the part that needs no device: the ABI surface of orbm_pnp_hypotheses (declared, exported, struct
mirrors = C layout, every refusal before the launch), the host instantiation of orb_slam2_e_amd/csrc/orbm_epnp.h
(orbm_debug_pnp_pose) against the literal restatement tests/pnp_oracle.c BIT FOR BIT, the restatement held to first principles --
planted inlier masks on integers, the restated double SVD / SVBkSb against numpy in float64 -- SetRansacParameters, the folds of
iterate with every quirk planted, the sensitivity to the SVD's hypot, and the Python / C++ classes without a device.

No OpenCV exists for this project to run: the restated cvSVD, cvInvert, cvSolve and cvMulTransposed are unpinned, like the other
OpenCV primitives."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_oracle as po
import pnp_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
SG = scenes.SIGMA2
OK, ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -5


@pytest.fixture(scope="module")
def so_path():
    return _lib.build()


# ------------------------------------------------------------------------------------------------ the ABI surface
def test_new_entry_points_are_declared_exported_and_bound(so_path):
    protos = _lib.prototypes()
    vp = C.c_void_p
    assert protos["orbm_pnp_hypotheses"] == (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp])
    assert protos["orbm_debug_last_pnp_waits"] == (C.c_int, [])
    assert protos["orbm_debug_pnp_pose"] == (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for name in ("orbm_pnp_hypotheses", "orbm_debug_last_pnp_waits", "orbm_debug_pnp_pose"):
        assert f" T {name}\n" in out
    L = _lib.lib()
    assert L.orbm_pnp_hypotheses.argtypes == protos["orbm_pnp_hypotheses"][1]
    assert L.orbx_abi_version() == 136


def test_struct_mirrors_have_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_pnp")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_pnp.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    m = pnp._CPnpProblem
    assert C.sizeof(m) == sizes["orbm_pnp_problem"]
    assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields["orbm_pnp_problem"]
    d = pnp.HYPOTHESIS_DTYPE
    assert d.itemsize == sizes["orbm_pnp_hypothesis"]
    assert [(k, d.fields[k][1], d.fields[k][0].itemsize) for k in d.names] == fields["orbm_pnp_hypothesis"]


def _call(problems, sigma2=SG, nlevels=None, P=None):
    L = _lib.lib()
    P = len(problems) if P is None else P
    arr = (pnp._CPnpProblem * max(len(problems), 1))(*[p.c() for p in problems])
    total = sum(p.H for p in problems)
    words = max(sum(p.H * ((p.n + 63) // 64) for p in problems), 1)
    hyp = np.zeros(max(total, 1), pnp.HYPOTHESIS_DTYPE); masks = np.zeros(words, np.uint64); rmasks = np.zeros(words, np.uint64)
    sg = np.ascontiguousarray(sigma2, np.float32)
    rc = L.orbm_pnp_hypotheses(arr, P, _lib.ptr(sg), len(sg) if nlevels is None else nlevels, None, _lib.ptr(hyp), _lib.ptr(masks), _lib.ptr(rmasks))
    return rc, L.orbm_debug_last_pnp_waits()


def _prob(n=12, H=4, **kw):
    p = scenes.problem(1, n, H)
    p.update(kw)
    return pnp.PnpProblem(p["Xw"], p["uv"], p["octave"], p["cam"], p["sets"], p["min_inliers"], p["th2"])


def test_every_refusal_comes_before_the_launch(so_path):
    import torch
    good = _prob()
    if torch.cuda.is_available():
        assert _call([good]) == (OK, 1)
    else:
        assert _call([good]) == (ERR_NO_DEVICE, 0)                           # valid input, no device: loud
        assert b"no usable HIP device" in _lib.lib().orbx_last_error()
    _check_refusals(good)


def _check_refusals(good):
    # limits
    assert _call([good] * 65)[0] == ERR_UNSUPPORTED
    assert _call([good], P=-1)[0] == ERR_ARG
    big_n = pnp.PnpProblem(np.zeros((8193, 3)), np.zeros((8193, 2)), np.zeros(8193), (1, 1, 0, 0), [[0, 1, 2, 3]], 8)
    assert _call([big_n])[0] == ERR_UNSUPPORTED
    big_h = _prob()
    big_h.sets = np.tile(big_h.sets[:1], (1025, 1)); big_h.H = 1025
    assert _call([big_h])[0] == ERR_UNSUPPORTED
    # nothing to do: OK, no launch, on any machine
    assert _call([]) == (OK, 0)
    assert _call([_prob(H=0), _prob(n=3, H=0)]) == (OK, 0)
    # argument errors
    three = _prob(n=3, H=0)
    three.sets = np.array([[0, 1, 2, 0]], np.int32); three.H = 1
    assert _call([three])[0] == ERR_ARG                                       # n < 4 with H > 0
    for bad in ([0, 1, 2, 12], [-1, 1, 2, 3], [0, 12, 2, 3]):                 # a set index outside [0, n)
        p = _prob(); p.sets[2] = bad
        assert _call([p])[0] == ERR_ARG and b"out of range" in _lib.lib().orbx_last_error()
    for v in (-1, scenes.NLEVELS):                                            # an octave outside [0, nlevels)
        p = _prob(); p.octave[7] = v
        assert _call([p])[0] == ERR_ARG and b"octave" in _lib.lib().orbx_last_error()
    p = _prob(); p.min_inliers = 0
    assert _call([p])[0] == ERR_ARG and b"min_inliers" in _lib.lib().orbx_last_error()
    assert _call([good, _prob(), three])[0] == ERR_ARG                        # the third problem of a batch
    assert _call([good], nlevels=0)[0] == ERR_ARG
    assert _lib.lib().orbm_debug_last_pnp_waits() == 0
    # the host entry
    L = _lib.lib()
    z = np.zeros(3 * 2049); cam = np.array(scenes.CAM); R = np.zeros(9); t = np.zeros(3); rep = np.zeros(1)
    args = lambda n: (_lib.ptr(z), _lib.ptr(z), n, _lib.ptr(cam), _lib.ptr(R), _lib.ptr(t), _lib.ptr(rep))
    assert L.orbm_debug_pnp_pose(*args(3)) == ERR_ARG and L.orbm_debug_pnp_pose(*args(2049)) == ERR_UNSUPPORTED
    assert L.orbm_debug_pnp_pose(None, *args(4)[1:]) == ERR_ARG


@pytest.mark.gpu
def test_refusals_with_a_device(so_path):
    _check_refusals(_prob())


def test_a_repeated_index_is_not_refused(so_path):
    """the fork's second iterate can draw a correspondence twice (:315): such a set passes validation (without a device the call
    then stops at the device check, not at an argument error)"""
    import torch
    p = _prob(); p.sets[1] = [3, 3, 5, 5]
    assert _call([p])[0] == (OK if torch.cuda.is_available() else ERR_NO_DEVICE)


# ------------------------------------------------------------------------------------------------ header == restatement, bit for bit
def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in arrays)


def _pose_cases():
    """(name, pws, us, expects a qr_solve early return): at least 200 random problems over the sizes, then the degenerate ones"""
    out = []
    for n in (4, 5, 6, 63, 64, 65, 130, 2048):
        for k in range(30 if n < 2048 else 4):
            q = scenes.problem(5000 + 31 * n + k, n, 0, outliers=0.25 if k % 3 else 0.0)
            out.append((f"n{n}_{k}", q["Xw"].astype(np.float64), q["uv"].astype(np.float64), False))
    q = scenes.problem(77, 30, 0, outliers=0.0)
    Xw, uv, _, sets = scenes.degenerate_sets(q, np.random.default_rng(3))
    names = ["repeated_twice", "four_times_the_same", "two_pairs", "coplanar", "collinear", "camera_centre", "nan_first", "nan_last"]
    for name, s in zip(names, sets):
        out.append((name, Xw[s].astype(np.float64), uv[s].astype(np.float64), name == "four_times_the_same"))
    return out


def test_host_header_equals_the_restatement_bit_for_bit(so_path):
    """orbm_debug_pnp_pose (hipcc's host pass over orbm_epnp.h) against tests/pnp_oracle.c (gcc): R, t and the reprojection error
    as bit patterns.  No tolerance: a difference is a bug in one of the two."""
    cases = _pose_cases()
    assert len(cases) >= 200 + 8
    singular = 0
    for name, pws, us, expects_singular in cases:
        R, t, rep, sing = po.pose(pws, us, scenes.CAM)
        R2, t2, rep2 = pnp.pnp_pose(pws, us, scenes.CAM)
        assert _bits(R, t, [rep]) == _bits(R2, t2, [rep2]), name
        if expects_singular:
            assert sing > 0, name                                      # qr_solve's "A is singular" early return is on the path
        singular += sing > 0
    assert singular >= 1
    # ordinary problems are solved: noise-free correspondences give the planted pose
    q = scenes.problem(91, 64, 0, outliers=0.0)
    R, t, rep = pnp.pnp_pose(q["Xw"], q["uv"], scenes.CAM)
    assert np.abs(R - q["R"]).max() < 1e-4 and np.abs(t - q["t"]).max() < 1e-3 and rep < 0.05


# ------------------------------------------------------------------------------------------------ the restated OpenCV primitives
@pytest.mark.parametrize("n", [3, 12])
def test_restated_double_svd_against_numpy(n):
    """well-conditioned symmetric positive definite inputs: singular values to 1e-12 relative, Ut rows up to sign to 1e-9"""
    rng = np.random.default_rng(40 + n)
    for _ in range(20):
        Q, _r = np.linalg.qr(rng.standard_normal((n, n)))
        w = np.sort(rng.uniform(1.0, 10.0, n))[::-1] * (1 + 0.3 * np.arange(n)[::-1])        # distinct, well separated
        A = (Q * w) @ Q.T
        A = (A + A.T) / 2
        W, Ut = po.svd_ut(A)
        U, S, _vt = np.linalg.svd(A)
        assert np.abs(W - S).max() <= 1e-12 * S.max()
        for i in range(n):
            assert min(np.abs(Ut[i] - U[:, i]).max(), np.abs(Ut[i] + U[:, i]).max()) < 1e-9, i
        assert np.abs(Ut @ Ut.T - np.eye(n)).max() < 1e-12


@pytest.mark.parametrize("nc", [3, 4, 5])
def test_restated_svbksb_against_lstsq(nc):
    rng = np.random.default_rng(50 + nc)
    for _ in range(20):
        A = rng.standard_normal((6, nc)); b = rng.standard_normal(6)
        x = po.solve_svd(A, b)
        ref = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.abs(x - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    A = rng.standard_normal((3, 3)) + 3 * np.eye(3)
    assert np.abs(po.invert_svd(A) - np.linalg.inv(A)).max() < 1e-9


# ------------------------------------------------------------------------------------------------ SetRansacParameters
def _ransac_restated(N, probability, minInliers, maxIterations, minSet, epsilon):
    """:123-159 in numpy scalars of the reference's types"""
    import math
    f32 = np.float32
    eps = f32(epsilon)
    n_min = max(int(f32(N) * eps), minInliers, minSet)
    if eps < f32(n_min) / f32(N):
        eps = f32(n_min) / f32(N)
    if n_min == N:
        its = 1
    else:
        den = math.log(1 - float(eps) ** 3) if eps < 1 else float("nan")
        v = math.log(1 - probability) / den if den == den and den != 0 else float("nan")
        its = int(math.ceil(v)) if v == v and abs(v) < 2 ** 31 else -2 ** 31
    return n_min, max(1, min(its, maxIterations)), float(eps)


@pytest.mark.parametrize("N", [4, 10, 19, 20, 21, 100, 1000])
def test_set_ransac_parameters(N):
    for args in ((0.99, 8, 300, 4, 0.4), (0.99, 10, 300, 4, 0.5), (0.99, 8, 50, 4, 0.4), (0.999, 4, 300, 4, 0.1), (0.99, 30, 300, 4, 0.4)):
        want = _ransac_restated(N, *args)
        assert po.ransac_parameters(N, *args) == pytest.approx(want, abs=0) and pnp.ransac_parameters(N, *args) == pytest.approx(want, abs=0), args
    # the truncation of N * epsilon, the float epsilon update, the clamp
    assert pnp.ransac_parameters(19, 0.99, 8, 300, 4, 0.4)[0] == 8 and pnp.ransac_parameters(21, 0.99, 8, 300, 4, 0.4)[0] == 8
    assert pnp.ransac_parameters(1000, 0.99, 8, 300, 4, 0.4)[0] == 400
    assert pnp.ransac_parameters(4, 0.99, 8, 300, 4, 0.4)[1] == 1             # more inliers asked for than correspondences


# ------------------------------------------------------------------------------------------------ first principles, on integers
def _non_coplanar(X):
    c = X - X.mean(0)
    s = np.linalg.svd(c.astype(np.float64), compute_uv=False)
    return s[2] > 0.05 * s[0]


#             name: (all-inlier sets whose mask is the planted one, records, hypothesis find() returns, its kind)
PINNED = {"n60": (56, [9, 11], 9, 1), "n130": (11, [19, 25], 19, 1), "n25": (139, [2, 3, 5], 2, 1)}


@pytest.mark.parametrize("flags", [po.DEFAULT, po.LIBM], ids=["own_hypot", "libm_hypot"])
def test_planted_inlier_masks(flags):
    """Refine on the planted mask returns a pose whose CheckInliers mask IS the planted mask; among the drawn sets at least one
    all-inlier set has the planted mask as its hypothesis mask; the fold returns the planted set.  Under both hypot builds."""
    for p in scenes.fold_scenes():
        planted = p["inlier"]
        assert planted.sum() >= 6 and _non_coplanar(p["Xw"][planted]), p["name"]
        R, t, rflags, cnt = po.refine(p, SG, planted, flags=flags)
        assert (rflags == planted).all() and cnt == planted.sum(), p["name"]
        h = po.hypotheses(p, SG, flags=flags)
        all_in = planted[p["sets"]].all(axis=1)
        exact = [k for k in np.flatnonzero(all_in) if (h["flags"][k] == planted).all()]
        records = [int(k) for k in np.flatnonzero(h["refined"])]
        s = po.Solver(p, SG, flags=flags)
        T, no_more, got, nin, hyp_index, kind = s.find()
        figures = (len(exact), records, hyp_index, kind)
        print(p["name"], flags[-1], "all-inlier sets", int(all_in.sum()), "figures", figures, "max_its", s.fold.max_its, "min", s.fold.min_inliers)
        assert len(exact) >= 1, p["name"]
        assert T is not None and (got == planted).all() and nin == planted.sum(), p["name"]
        if flags == po.DEFAULT:
            assert figures == PINNED[p["name"]], p["name"]
        # every record's Refine mask on these scenes is the planted mask or a subset of it (outliers are 20 px away)
        for k in records:
            assert not (h["rflags"][k] & ~planted).any()


def test_check_inliers_types():
    """strict < against sigma2 * th2, NaN is never an inlier, the planted pose takes exactly the planted inliers"""
    p = scenes.fold_scenes()[0]
    flags, cnt = po.check_inliers(p["R"], p["t"], p, SG)
    assert (flags == p["inlier"]).all() and cnt == p["inlier"].sum()
    q = dict(p, Xw=p["Xw"].copy()); q["Xw"][5, 1] = np.nan
    flags, _ = po.check_inliers(p["R"], p["t"], q, SG)
    assert not flags[5]
    # a pixel displaced so that error2 == the float threshold exactly is outside; just below is inside
    one = dict(p, n=1, Xw=np.array([[0, 0, 4]], np.float32), uv=np.zeros((1, 2), np.float32), octave=np.array([0], np.int32), cam=(1.0, 1.0, 0.0, 0.0),
               th2=np.float32(4.0))
    for dx, want in ((2.0, False), (np.nextafter(np.float32(2.0), np.float32(0)), True)):
        one["uv"] = np.array([[dx, 0]], np.float32)
        assert bool(po.check_inliers(np.eye(3), np.zeros(3), one, SG)[0][0]) == want


# ------------------------------------------------------------------------------------------------ the folds
def _fold(N=100, min_inliers=8, max_its=20):
    return po.Fold(N, min_inliers, max_its, 0, 0, -1, 0.0, 0)


def _iterate(f, counts, nrefined, n):
    counts = np.ascontiguousarray(counts, np.int32); nrefined = np.ascontiguousarray(nrefined, np.int32)
    no_more, nin, kind = C.c_int(0), C.c_int(0), C.c_int(0)
    h = po.lib().pno_iterate(C.byref(f), po._p(counts), po._p(nrefined), len(counts), n, C.byref(no_more), C.byref(nin), C.byref(kind))
    return h, bool(no_more.value), nin.value, kind.value


def test_fold_quirks_planted():
    z = np.zeros(40, np.int32)
    # the first iterate(5) runs every remaining iteration up to the maximum; each later call runs five more
    f = _fold()
    assert _iterate(f, z, z, 5) == (-1, True, 0, 0) and f.iterations == 20
    assert _iterate(f, z, z, 5) == (-1, True, 0, 0) and f.iterations == 25
    assert _iterate(f, z, z, 5)[0] == -1 and f.iterations == 30
    # Refine at exactly min inliers does not return (strict >); the best is returned at the end with bNoMore
    c = z.copy(); r = z.copy(); c[3] = 12; r[3] = 8
    f = _fold()
    assert _iterate(f, c, r, 5) == (3, True, 12, 2) and f.iterations == 20 and f.best_inliers == 12
    # ... at min + 1 it returns at once, bNoMore false
    r[3] = 9
    f = _fold()
    assert _iterate(f, c, r, 5) == (3, False, 9, 1) and f.iterations == 4
    # the carried best: an equal count later does not replace the best (>), a larger one does; >= enters the block
    c = z.copy(); r = z.copy(); c[2] = 10; r[2] = 5; c[6] = 10; r[6] = 30; c[25] = 11; r[25] = 9
    f = _fold()
    assert _iterate(f, c, r, 5) == (2, True, 10, 2) and f.best == 2          # hypothesis 6 (equal count) is no record: its nrefined is never read
    f = _fold()
    _iterate(f, c, r, 5)
    assert f.best_inliers == 10 and f.iterations == 20
    assert _iterate(f, c, r, 5)[0] == 2 and f.iterations == 25               # 20 .. 24: nothing new, the carried best again
    assert _iterate(f, c, r, 5) == (25, False, 9, 1) and f.best_inliers == 11 and f.iterations == 26
    # N < min: bNoMore and nothing else
    f = _fold(N=7)
    assert _iterate(f, z, z, 5) == (-1, True, 0, 0) and f.iterations == 0


def _oracle_backed(problems, level_sigma2, best_in=None):
    """pnp.pnp_hypotheses computed by the restatement: what the device returns, for folds run without one"""
    out = []
    for k, p in enumerate(problems):
        d = dict(Xw=p.Xw, uv=p.uv, octave=p.octave, sets=p.sets, n=p.n, H=p.H, cam=p.cam, th2=p.th2, min_inliers=p.min_inliers)
        o = po.hypotheses(d, level_sigma2, 0 if best_in is None else int(best_in[k]))
        hyp = np.zeros(p.H, pnp.HYPOTHESIS_DTYPE)
        for f in ("R", "t", "rep_error", "ninliers", "refined", "Rr", "tr", "nrefined"):
            hyp[f] = o[f]
        out.append((hyp, po.masks_of(o["flags"]), po.masks_of(o["rflags"])))
    return out


def _solver(p, **kw):
    return pnp.PnPsolver(p["Xw"], p["uv"], p["octave"], p["cam"], SG, sets=p["sets"], **kw)


@pytest.mark.parametrize("calls", [[300], [5, 5, 5, 5], [1, 400, 3]])
def test_python_class_folds_like_the_restatement(monkeypatch, calls):
    """orb_slam2_e_amd.PnPsolver over restatement-computed hypotheses against the restatement's own fold (pno_iterate), call by call:
    Tcw, bNoMore, the inlier vector scattered through mvKeyPointIndices, the count, mnIterations and mnBestInliers"""
    monkeypatch.setattr(pnp, "pnp_hypotheses", _oracle_backed)
    for p, (min_in, max_its) in zip(scenes.fold_scenes(), ((8, 300), (60, 12), (30, 300))):
        p = dict(p, sets=scenes.draw_sets(np.random.default_rng(5), p["n"], 1024))
        idx = np.arange(p["n"]) * 2 + 1
        s = _solver(p, indices=idx, n_matches=2 * p["n"] + 3); s.SetRansacParameters(0.99, min_in, max_its)
        o = po.Solver(p, SG, minInliers=min_in, maxIterations=max_its)
        assert (s.mRansacMinInliers, s.mRansacMaxIts) == (o.fold.min_inliers, o.fold.max_its)
        for n in calls:
            T, no_more, inl, nin = s.iterate(n)
            To, no_more_o, flags_o, nin_o, _h, _kind = o.iterate(n)
            assert (T is None) == (To is None) and no_more == no_more_o and nin == nin_o, (p["name"], n)
            assert (s.mnIterations, s.mnBestInliers) == (o.fold.iterations, o.fold.best_inliers)
            assert inl.shape == (2 * p["n"] + 3,)
            if T is not None:
                assert T.dtype == np.float32 and T.tobytes() == To.tobytes()
                assert (np.flatnonzero(inl) == idx[flags_o]).all()
            else:
                assert not inl.any()


def test_python_class_small_cases(monkeypatch):
    monkeypatch.setattr(pnp, "pnp_hypotheses", _oracle_backed)
    p = scenes.problem(3, 7, 10)
    s = _solver(p)
    assert s.mRansacMinInliers == 8
    T, no_more, inl, nin = s.iterate(5)
    assert T is None and no_more and nin == 0 and not inl.any() and s.mnIterations == 0       # N < min: bNoMore, no evaluation
    # two solvers evaluated together return what each returns alone
    a, b = scenes.fold_scenes()[0], scenes.fold_scenes()[2]
    sa, sb = _solver(a), _solver(b)
    pnp.PnPsolver.evaluate([sa, sb])
    for s, q in ((sa, a), (sb, b)):
        alone = _solver(q)
        ra, rb = s.find(), alone.find()
        assert ra[0].tobytes() == rb[0].tobytes() and (ra[1] == rb[1]).all() and ra[2] == rb[2]
    with pytest.raises(ValueError):
        pnp.PnPsolver(a["Xw"], a["uv"], a["octave"], a["cam"], SG)
    with pytest.raises(ValueError):
        _solver(a).SetRansacParameters(minSet=5)


def test_frame_stage1_fold(monkeypatch):
    """the first stage of iterate(Frame &, ..): the fork's draw rule (sets may repeat an index), the recorded poses, and the
    accept callback deciding a successful Refine -- against pno_iterate_frame_stage1"""
    monkeypatch.setattr(pnp, "pnp_hypotheses", _oracle_backed)
    rng = np.random.default_rng(17)
    sets = pnp.draw_sets(12, 400, lambda lo, hi: int(rng.integers(lo, hi + 1)), frame_rule=True)
    assert (np.sort(sets, axis=1)[:, 1:] == np.sort(sets, axis=1)[:, :-1]).any()              # the rule does repeat correspondences
    assert (sets == scenes.draw_sets(np.random.default_rng(17), 12, 400, frame_rule=True)).all()
    for accept_all in (True, False):
        p = scenes.problem(29, 60, 300, frame_rule=True)
        s = _solver(p); s.SetRansacParameters(0.99, 20, 300)
        seen = []
        T, inl, nin, poses = s.iterate_frame_stage1(5, lambda R, t: (seen.append((R, t)), accept_all)[1])
        f = po.Fold(p["n"], 0, 0, 0, 0, -1, 0.0, 0)
        po.lib().pno_set_ransac_parameters(C.byref(f), 0.99, 20, 300, 4, 0.4)
        o = po.hypotheses(dict(p, min_inliers=f.min_inliers), SG)
        accept = np.full(300, int(accept_all), np.uint8); out = np.zeros(300, np.int32); npos = C.c_int(0)
        h = po.lib().pno_iterate_frame_stage1(C.byref(f), po._p(o["ninliers"]), po._p(o["nrefined"]), po._p(accept), 300, 5, po._p(out), C.byref(npos))
        assert (T is not None) == (h >= 0) == accept_all
        assert [(c, it) for _, _, c, it in poses] == [(int(o["ninliers"][k]), int(k)) for k in out[:npos.value]] and s.mnIterations == f.iterations
        for (R, t, _, _), k in zip(poses, out[:npos.value]):
            assert R.tobytes() == o["R"][k].tobytes() and t.tobytes() == o["t"][k].tobytes()
        if accept_all:
            assert T.tobytes() == po.tcw(o["Rr"][h], o["tr"][h]).tobytes() and nin == o["nrefined"][h] and (inl == o["rflags"][h]).all()
            assert len(seen) == 1 and seen[0][0].tobytes() == o["Rr"][h].tobytes()
        else:
            assert len(seen) >= 1 and not inl.any() and nin == 0


# ------------------------------------------------------------------------------------------------ hypot sensitivity (reported)
def test_hypot_sensitivity_is_reported():
    """The share of hypotheses whose mask differs between the SVD with this project's hypot and with libm's, and the largest pose
    difference among the rest (DESIGN 22 quotes both).  Not gating: the gating part is test_planted_inlier_masks under both builds."""
    differ = total = 0
    worst = 0.0
    for p in scenes.fold_scenes():
        a, b = po.hypotheses(p, SG, flags=po.DEFAULT), po.hypotheses(p, SG, flags=po.LIBM)
        same = (a["flags"] == b["flags"]).all(axis=1)
        differ += int((~same).sum()); total += p["H"]
        for k in np.flatnonzero(same):
            Ta, Tb = np.concatenate([a["R"][k], a["t"][k]]), np.concatenate([b["R"][k], b["t"][k]])
            if np.isfinite(Ta).all() and np.isfinite(Tb).all():
                worst = max(worst, float(np.abs(Ta - Tb).max() / max(1.0, np.abs(Ta).max())))
    print(f"hypot sensitivity: {differ} of {total} hypothesis masks differ; largest relative pose difference among the rest {worst:.3g}")
    assert total == 900


# ------------------------------------------------------------------------------------------------ the C++ class and the shell
def write_scene(path, p, min_inliers, max_its, calls, stride=1, extra=0):
    """a scene file for tests/cxx/pnp_smoke.cpp; the correspondences stand at every `stride`-th place of vpMapPointMatches"""
    n, sets = p["n"], np.asarray(p["sets"]).reshape(-1, 4)
    with open(path, "w") as f:
        f.write(f"{n} {stride * n + extra} {len(sets)} {p['cam'][0]!r} {p['cam'][1]!r} {p['cam'][2]!r} {p['cam'][3]!r} {min_inliers} {max_its} {len(calls)}\n")
        f.write(" ".join(str(c) for c in calls) + f"\n{len(SG)} " + " ".join(f"{v:.9g}" for v in SG) + "\n")
        for i in range(n):
            f.write(" ".join(f"{v:.9g}" for v in (*p["Xw"][i], *p["uv"][i])) + f" {p['octave'][i]} {stride * i}\n")
        for s in sets:
            f.write(" ".join(str(v) for v in s) + "\n")


def build_smoke(tmp_path):
    _lib.build()
    exe = str(tmp_path / "pnp_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "pnp_smoke.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_class_fails_loudly_without_a_device(tmp_path):
    """on a machine without a device the first iterate() returns ORBX_ERR_NO_DEVICE cleanly (with one, it runs)"""
    import torch
    gpu = torch.cuda.is_available()
    scene = str(tmp_path / "scene.txt")
    write_scene(scene, scenes.fold_scenes()[0], 8, 300, [5])
    out = subprocess.run([build_smoke(tmp_path)] + ([] if gpu else ["nodevice"]) + [scene], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ("OK 1 solvers" if gpu else "OK nodevice") in out.stdout


def test_integration_shell_calls_the_declared_entry_points():
    """integration/PnPsolver_ransac_hip.cc cannot be compiled here (no OpenCV / DBoW2): the library calls it makes have the declared
    numbers of arguments, every ORBM_ / ORBX_ constant it names exists, and the documents list it"""
    import test_cpu_integration_shells as shells
    decl, header_text = shells._declarations()
    src = open(os.path.join(ROOT, "integration", "PnPsolver_ransac_hip.cc")).read()
    calls = [c for c in shells._calls(src) if c[0] in decl]
    assert all(decl[f] == n for f, n in calls), calls
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", shells._strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    # the shell goes through the C++ class, whose library calls are checked the same way
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    body = hpp[hpp.index("class PnPsolver {"):hpp.index("// Optimizer::OptimizeSim3 (src/Optimizer.cc")]
    calls = [c for c in shells._calls(body) if c[0] in decl]
    assert calls and all(c == ("orbm_pnp_hypotheses", 8) for c in calls) and decl["orbm_pnp_hypotheses"] == 8
    stripped = shells._strip_comments(src)
    assert "orbslam_hip::PnPsolver" in stripped and "iterateFrameStage1" in stripped and "PnPsolverHipProjectBestPoses" in src
    assert "PnPsolver_ransac_hip.cc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "PnPsolver_ransac_hip.cc" in open(os.path.join(ROOT, "integration", "README.md")).read()
