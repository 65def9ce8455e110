"""Sim3Solver on the device, the part that needs no device: the ABI surface of orbm_sim3_hypotheses (declared, exported, struct
mirrors = C layout, every refusal before the launch), the CPU restatement (tests/sim3_oracle.c) held to first principles -- exact
synthetic similarities, the restated cv::eigen against numpy in float64, cv::Rodrigues against its closed form, the truncated
integer thresholds -- the fold of iterate on hand-made count sequences, the scenes' share of near-threshold flags, and the C++
class without a device.

No OpenCV exists for this project to run: the restated JacobiImpl_<float> and cvRodrigues2 are unpinned, like the other OpenCV
primitives."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_oracle as so
import sim3_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import sim3 as s3

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
    assert protos["orbm_sim3_hypotheses"] == (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp])
    assert protos["orbm_debug_last_sim3_waits"] == (C.c_int, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for name in ("orbm_sim3_hypotheses", "orbm_debug_last_sim3_waits"):
        assert f" T {name}\n" in out
    L = _lib.lib()
    assert L.orbm_sim3_hypotheses.argtypes == protos["orbm_sim3_hypotheses"][1]
    assert L.orbx_abi_version() == 136


def test_struct_mirrors_have_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_sim3")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_sim3.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    m = s3._CSim3Problem
    assert C.sizeof(m) == sizes["orbm_sim3_problem"]
    assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields["orbm_sim3_problem"]
    d = s3.HYPOTHESIS_DTYPE
    assert d.itemsize == sizes["orbm_sim3_hypothesis"]
    assert [(k, d.fields[k][1], d.fields[k][0].itemsize) for k in d.names] == fields["orbm_sim3_hypothesis"]


def _call(problems, sigma2=SG, nlevels=None, P=None):
    L = _lib.lib()
    P = len(problems) if P is None else P
    arr = (s3._CSim3Problem * max(len(problems), 1))(*[p.c() for p in problems])
    total = sum(p.H for p in problems)
    hyp = np.zeros(max(total, 1), s3.HYPOTHESIS_DTYPE); masks = np.zeros(max(sum(p.H * ((p.n + 63) // 64) for p in problems), 1), np.uint64)
    sg = np.ascontiguousarray(sigma2, np.float32)
    rc = L.orbm_sim3_hypotheses(arr, P, _lib.ptr(sg), len(sg) if nlevels is None else nlevels, _lib.ptr(hyp), _lib.ptr(masks))
    return rc, L.orbm_debug_last_sim3_waits()


def _prob(n=10, H=4, **kw):
    p = scenes.problem(1, n, H)
    p.update(kw)
    return s3.Sim3Problem(p["X1w"], p["X2w"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"], p["triples"], p["fix_scale"])


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
    big_n = s3.Sim3Problem(np.zeros((8193, 3)), np.zeros((8193, 3)), np.zeros(8193), np.zeros(8193), np.eye(4), np.eye(4), (1, 1, 0, 0), (1, 1, 0, 0),
                           [[0, 1, 2]])
    assert _call([big_n])[0] == ERR_UNSUPPORTED
    big_h = _prob()
    big_h.triples = np.tile(big_h.triples[:1], (1025, 1)); big_h.H = 1025
    assert _call([big_h])[0] == ERR_UNSUPPORTED
    # nothing to do: OK, no launch, on any machine
    assert _call([]) == (OK, 0)
    assert _call([_prob(H=0), _prob(n=2, H=0)]) == (OK, 0)
    # argument errors
    two = _prob(n=2, H=0)
    two.triples = np.array([[0, 1, 0]], np.int32); two.H = 1
    assert _call([two])[0] == ERR_ARG                                         # n < 3 with H > 0
    for bad in ([0, 1, 10], [-1, 1, 2], [0, 10, 2]):                          # a triple index outside [0, n)
        p = _prob(); p.triples[2] = bad
        assert _call([p])[0] == ERR_ARG and b"out of range" in _lib.lib().orbx_last_error()
    for bad in ([3, 3, 5], [3, 5, 3], [5, 3, 3]):                             # a repeated index
        p = _prob(); p.triples[1] = bad
        assert _call([p])[0] == ERR_ARG and b"repeats" in _lib.lib().orbx_last_error()
    for field in ("octave1", "octave2"):                                      # an octave outside [0, nlevels)
        for v in (-1, scenes.NLEVELS):
            p = _prob(); getattr(p, field)[7] = v
            assert _call([p])[0] == ERR_ARG and b"octave" in _lib.lib().orbx_last_error()
    assert _call([good, _prob(), two])[0] == ERR_ARG                          # the third problem of a batch
    assert _call([good], nlevels=0)[0] == ERR_ARG
    assert _lib.lib().orbm_debug_last_sim3_waits() == 0


# ------------------------------------------------------------------------------------------------ the restatement from first principles
def _non_degenerate(Xc, tri):
    """the triangle's smallest height is at least a fifth of its longest side: a triple that fixes the rotation well"""
    a, b, c = (Xc[tri[:, k]].astype(np.float64) for k in range(3))
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    longest = np.maximum(np.maximum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1)), np.linalg.norm(c - b, axis=1))
    return area2 / longest ** 2 >= 0.2


@pytest.mark.parametrize("fix_scale", [False, True])
def test_noiseless_pairs_return_the_similarity(fix_scale):
    """s = 1.7 (1 with the scale fixed), 40 degrees about a skew axis, t != 0: every non-degenerate triple returns R, t, s to 1e-4
    relative, and all n points are inliers"""
    p = scenes.problem(31, 80, 300, fix_scale=fix_scale)
    assert p["s"] == (1.0 if fix_scale else 1.7) and np.linalg.norm(p["t"]) > 0.5
    h = so.hypotheses(p, SG)
    ok = _non_degenerate(h["pre"]["Xc1"], p["triples"])
    assert ok.sum() > 150
    R = h["R12"].reshape(-1, 3, 3).astype(np.float64)
    eR = np.linalg.norm(R - p["R"], axis=(1, 2)) / np.linalg.norm(p["R"])
    et = np.linalg.norm(h["t12"] - p["t"], axis=1) / np.linalg.norm(p["t"])
    es = np.abs(h["s12"].astype(np.float64) - p["s"]) / p["s"]
    print("fix_scale", fix_scale, "largest relative error of R, t, s over", int(ok.sum()), "triples:", eR[ok].max(), et[ok].max(), es[ok].max())
    assert eR[ok].max() <= 1e-4 and et[ok].max() <= 1e-4 and es[ok].max() <= 1e-4
    assert (h["ninliers"][ok] == p["n"]).all() and h["flags"][ok].all()
    if fix_scale:
        assert (h["s12"] == 1.0).all()
    # T12 is [sR | t; 0 0 0 1]
    T = h["T12"].reshape(-1, 4, 4)
    assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(T), 1))) and np.array_equal(T[:, :3, 3], h["t12"])
    assert np.allclose(T[:, :3, :3], h["s12"][:, None, None] * h["R12"].reshape(-1, 3, 3), rtol=1e-6, atol=0)


def test_restated_eigen_against_numpy():
    """N q = lambda q to 1e-5 (relative to the largest |lambda|), lambda descending, the leading eigenvector = numpy's eigh in
    float64 up to sign"""
    rng = np.random.default_rng(2)
    mats = []
    p = scenes.problem(32, 60, 100, noise=1.0, outliers=0.3)
    pre = so.prepare(p, SG)
    for tri in p["triples"]:
        mats.append(so.compute_sim3(pre["Xc1"][tri], pre["Xc2"][tri])["N"])
    for _ in range(50):
        A = rng.standard_normal((4, 4)); mats.append(((A + A.T) / 2).astype(np.float32))
    mats.append(np.diag([1.0, 4.0, -2.0, 3.0]).astype(np.float32))
    worst_res = worst_vec = 0.0
    for N in mats:
        assert np.array_equal(N, N.T)
        w, V, rotations = so.eigen4(N)
        assert rotations < 480 and (np.diff(w) <= 0).all()
        N64 = N.astype(np.float64); scale = max(np.abs(w).max(), 1e-30)
        res = np.abs(N64 @ V.T.astype(np.float64) - V.T.astype(np.float64) * w.astype(np.float64)).max() / scale
        w64, V64 = np.linalg.eigh(N64)
        assert np.allclose(w, w64[::-1], rtol=0, atol=1e-5 * scale)
        lead = V64[:, -1]
        dv = min(np.linalg.norm(V[0] - lead), np.linalg.norm(V[0] + lead))
        gap = (w64[-1] - w64[-2]) / scale
        assert res <= 1e-5, res
        assert dv <= 1e-5 / max(gap, 1e-3), (dv, gap)           # float accuracy over the gap to the next eigenvalue
        worst_res = max(worst_res, res); worst_vec = max(worst_vec, dv)
    print("restated cv::eigen over", len(mats), "matrices: largest residual", worst_res, "largest eigenvector difference", worst_vec)
    w, V, rotations = so.eigen4(np.diag([1.0, 4.0, -2.0, 3.0]))
    assert rotations == 0 and np.array_equal(w, [4, 3, 1, -2]) and np.array_equal(V[0], [0, 1, 0, 0])


def test_restated_rodrigues_against_the_closed_form():
    rng = np.random.default_rng(3)
    vecs = [rng.standard_normal(3) * a for a in (1e-3, 0.1, 1.0, 3.0, 6.0) for _ in range(10)] + [[np.pi, 0, 0], [0, 0, 2 * np.pi]]
    for v in vecs:
        v32 = np.asarray(v, np.float32); v64 = v32.astype(np.float64)
        th = np.linalg.norm(v64); r = v64 / th
        K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        R64 = np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(r, r) + np.sin(th) * K
        assert np.abs(so.rodrigues(v32) - R64).max() <= 2 ** -23                    # the rounding to float and a few double ulps
    assert np.array_equal(so.rodrigues([0, 0, 0]), np.eye(3))                         # theta < DBL_EPSILON: the identity
    assert np.array_equal(so.rodrigues([1e-17, 0, 0]), np.eye(3))
    assert np.isnan(so.rodrigues([np.nan, np.nan, np.nan])).all()                     # what the identity rotation hands it (0 / 0 at :280)
    X = (np.random.default_rng(4).random((3, 3)) + 2).astype(np.float32)
    out = so.compute_sim3(X, X)
    assert np.isnan(out["T12"][:3]).all() and np.isnan(out["R12"]).all() and np.isnan(out["s12"])


def test_truncated_integer_thresholds():
    """mvnMaxError is a vector of size_t: 9.210 * 1.44 = 13.26 is stored as 13, and err < 13 compares floats"""
    assert so.max_error(1.44) == 13 and so.max_error(1.0) == 9 and so.max_error(np.float32(1.2) ** 14) == int(9.210 * float(np.float32(1.2) ** 14))
    below = np.nextafter(np.float32(13), np.float32(0))
    assert not so.is_inlier(13.0, 0.0, 13, 13) and not so.is_inlier(0.0, 13.0, 13, 13)
    assert so.is_inlier(below, below, 13, 13)
    assert not so.is_inlier(13.2, 0.0, 13, 13)                                       # inside 13.26, outside the stored 13
    assert not so.is_inlier(np.nan, 0.0, 13, 13) and not so.is_inlier(0.0, np.inf, 13, 13)
    pre = so.prepare(scenes.problem(1, 16, 1), SG)
    p = scenes.problem(1, 16, 1)
    assert np.array_equal(pre["max1"], [int(9.210 * float(SG[o])) for o in p["octave1"]])


# ------------------------------------------------------------------------------------------------ the fold
def _fold(counts, N, min_inliers, max_its):
    return so.Fold(N, min_inliers, max_its, 0, 0, -1), np.asarray(counts, np.int32)


def _it(f, c, n):
    no_more, nin = C.c_int(0), C.c_int(0)
    h = so.lib().s3o_iterate(C.byref(f), c.ctypes.data_as(C.c_void_p), n, C.byref(no_more), C.byref(nin))
    return h, bool(no_more.value), nin.value


def test_fold_on_hand_made_count_sequences():
    # the first count > min succeeds (== min does not: the comparison is strict)
    f, c = _fold([3, 6, 5, 7, 2], 10, 6, 5)
    assert _it(f, c, 5) == (3, False, 7) and f.iterations == 4 and f.best_inliers == 7
    # of equal bests the last wins (>=), without success below min
    f, c = _fold([4, 2, 4, 1], 10, 6, 4)
    assert _it(f, c, 4) == (-1, True, 0) and f.best == 2 and f.best_inliers == 4
    # after a success only >= best succeeds: 8, then 7 is passed over, 8 again succeeds, 9 succeeds
    f, c = _fold([8, 7, 8, 9, 7], 10, 6, 5)
    assert _it(f, c, 1) == (0, False, 8)
    assert _it(f, c, 1) == (-1, False, 0) and f.best == 0
    assert _it(f, c, 1) == (2, False, 8)
    assert _it(f, c, 5) == (3, False, 9)
    assert _it(f, c, 5) == (-1, True, 0) and f.iterations == 5 and f.best == 3
    # bNoMore exactly when mnIterations >= mRansacMaxIts: a success on the last iteration does not set it
    f, c = _fold([1, 1, 9], 10, 6, 3)
    assert _it(f, c, 2) == (-1, False, 0)
    assert _it(f, c, 1) == (2, False, 9)
    assert _it(f, c, 1) == (-1, True, 0)
    # rounds of five
    f, c = _fold([0] * 12, 10, 6, 12)
    assert [_it(f, c, 5)[1] for _ in range(3)] == [False, False, True]
    # N < minInliers returns at once
    f, c = _fold([9, 9], 5, 6, 2)
    assert _it(f, c, 5) == (-1, True, 0) and f.iterations == 0


def test_ransac_parameters():
    """mRansacMaxIts of :120-137, and the Python class computes the same"""
    assert so.ransac_max_its(0.99, 6, 300, 6) == 1                     # minInliers == N
    assert so.ransac_max_its(0.99, 6, 300, 20) == int(np.ceil(np.log(0.01) / np.log(1 - float(np.float32(6) / np.float32(20)) ** 3)))
    assert so.ransac_max_its(0.99, 6, 300, 1000) == 300 and so.ransac_max_its(0.99, 20, 300, 5) == 1 and so.ransac_max_its(0.99, 6, 300, 0) == 1
    for N in list(range(0, 40)) + [100, 1000, 8192]:
        for m in (0, 3, 6, 20):
            for prob, mx in ((0.99, 300), (0.5, 10), (0.999, 1000)):
                assert s3.ransac_max_iterations(prob, m, mx, N) == so.ransac_max_its(prob, m, mx, N), (N, m, prob, mx)


def test_draw_loop():
    """:163-177: the drawn entry is replaced by the last of the list; three distinct indices"""
    seq = iter([0, 0, 0, 4, 3, 2])
    tri = s3.draw_triples(5, 2, lambda lo, hi: next(seq))
    assert tri.tolist() == [[0, 4, 3], [4, 3, 2]]
    import random
    r = random.Random(1)
    tri = s3.draw_triples(7, 200, r.randint)
    assert ((tri >= 0) & (tri < 7)).all() and (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
    assert np.array_equal(tri, so.draw_triples(7, 200, random.Random(1).randint))


# ------------------------------------------------------------------------------------------------ margin rule and class
def test_scenes_keep_near_threshold_flags_under_the_cap():
    """At most 2 % of a scene's (hypothesis, point) flags have a relative gap under 1e-3 to either threshold in the restatement
    alone: the device test may then exclude flags under any M <= 1e-3 and stay inside its cap of 2 % (both figures: the project's
    rule, tests/test_gpu_create_points.py and DESIGN 12)"""
    for p in scenes.restatement_scenes():
        h = so.hypotheses(p, SG)
        low = int((h["gap"] < 1e-3).sum())
        print(p["name"], "flags", h["gap"].size, "gap < 1e-3:", low, "best count", int(h["ninliers"].max()))
        assert low <= 0.02 * h["gap"].size, p["name"]
        assert h["ninliers"].max() > 6                                   # the scenes are loop closures that succeed


def _build_smoke(tmp_path):
    _lib.build()
    exe = str(tmp_path / "sim3_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "sim3_smoke.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_class_fails_loudly_without_a_device(tmp_path):
    """on a machine without a device the first iterate() returns ORBX_ERR_NO_DEVICE cleanly (with one, the program's device run)"""
    import torch
    gpu = torch.cuda.is_available()
    out = subprocess.run([_build_smoke(tmp_path)] + ([] if gpu else ["nodevice"]), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ("OK two candidates" if gpu else "OK nodevice") in out.stdout


@pytest.mark.gpu
def test_cxx_class_on_the_device(tmp_path):
    out = subprocess.run([_build_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK")


@pytest.mark.gpu
def test_refusals_with_a_device(so_path):
    _check_refusals(_prob())


def test_integration_shell_calls_the_declared_entry_points():
    """integration/Sim3Solver_hip.cc cannot be compiled here (no OpenCV / DBoW2): the library calls it makes have the declared
    numbers of arguments, every ORBM_ / ORBX_ constant it names exists, and the documents list it"""
    import test_cpu_integration_shells as shells
    decl, header_text = shells._declarations()
    src = open(os.path.join(ROOT, "integration", "Sim3Solver_hip.cc")).read()
    calls = [c for c in shells._calls(src) if c[0] in decl]
    assert all(decl[f] == n for f, n in calls), calls
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", shells._strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    # the shell goes through the C++ class, whose one library call is checked the same way
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    body = hpp[hpp.index("class Sim3Solver {"):]
    assert ("orbm_sim3_hypotheses", 6) in [c for c in shells._calls(body) if c[0] in decl] and decl["orbm_sim3_hypotheses"] == 6
    assert "orbslam_hip::Sim3Solver" in shells._strip_comments(src)
    assert "Sim3Solver_hip.cc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Sim3Solver_hip.cc" in open(os.path.join(ROOT, "integration", "README.md")).read()
