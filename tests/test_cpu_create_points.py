"""LocalMapping::CreateNewMapPoints in one call, the part that needs no device: the CPU restatement (tests/create_points_oracle.c)
held to first principles in float64 numpy -- the restated cv::SVD gives the null vector, the gates recomputed in float64 agree on
every pair that is not within 1e-3 of a threshold, planted pairs get their status -- the scenes' share of near-threshold pairs,
and the ABI surface of orbm_create_new_map_points (declared, exported, struct mirror = C layout, refusals before the launch).

No OpenCV exists for this project to run: the restated JacobiSVDImpl_<float> is unpinned, like the other OpenCV primitives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import create_points_oracle as cpo
import create_points_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd.matcher import ORBmatcher, _CTriangKeyFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST = cpo.STATUS


@pytest.fixture(scope="module")
def restated():
    """the restatement's run of every scene, computed once"""
    return [(s, cpo.create_new_map_points(s)) for s in scenes.restatement_scenes()]


# ------------------------------------------------------------------------------------------------ the restated SVD
def test_restated_svd_gives_the_null_vector_of_triangulation_matrices(restated):
    """vt.row(3) against numpy's float64 SVD of the same float matrix: same direction to float accuracy times the conditioning
    (gap between the two smallest singular values), unit length, and the sweep count stays far from the cap of 30."""
    worst = 0.0; n = 0
    for s, r in restated:
        for A in r["A"][r["from_svd"]]:
            v, sweeps = cpo.svd_vt3(A)
            assert 1 <= sweeps <= 12
            U, w, Vt = np.linalg.svd(A.astype(np.float64).reshape(4, 4))
            assert abs(np.linalg.norm(v.astype(np.float64)) - 1) < 1e-5
            err = min(np.linalg.norm(v - Vt[3]), np.linalg.norm(v + Vt[3]))
            # a perturbation of A of relative size eps_float turns the null vector by about eps * w[0] / (w[2] - w[3])
            assert err < 32 * np.finfo(np.float32).eps * w[0] / (w[2] - w[3]), (err, w)
            worst = max(worst, err); n += 1
    assert n > 400
    print("restated SVD: largest |v - v64| over", n, "matrices:", worst)


def test_restated_svd_on_known_matrices():
    # diagonal: already orthogonal columns -- no rotation, the row of the smallest column norm comes last
    v, sweeps = cpo.svd_vt3(np.diag([3.0, 0.5, 2.0, 1.0]))
    assert sweeps == 1 and np.array_equal(v, [0, 1, 0, 0])
    # an exact null vector with integer entries
    x = np.array([1.0, -2.0, 2.0, 4.0])
    rng = np.random.default_rng(1)
    B = rng.integers(-4, 5, (4, 4)).astype(np.float64)
    B -= np.outer(B @ x, x) / (x @ x)
    v, _ = cpo.svd_vt3(B.astype(np.float32))
    assert np.allclose(v[:3] / v[3], x[:3] / x[3], rtol=0, atol=2e-6)
    # the zero matrix: nothing to rotate, every singular value 0, no swap -- the last row of the identity
    v, sweeps = cpo.svd_vt3(np.zeros((4, 4)))
    assert sweeps == 1 and np.array_equal(v, [0, 0, 0, 1])


# ------------------------------------------------------------------------------------------------ the gates in float64
def _status64(scene, k, i1, i2):
    """LocalMapping.cc:338-497 in float64 with a float64 SVD: the status a pair has when no rounding is near a threshold"""
    cur, nb = scene["cur"], scene["neigh"][k]
    T1, T2 = cur["Tcw"].astype(np.float64), nb["Tcw"].astype(np.float64)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    fx1, fy1, cx1, cy1, mb1, mbf1 = (float(v) for v in cur["cam"]); fx2, fy2, cx2, cy2, mb2, _ = (float(v) for v in nb["cam"])
    kp1, kp2 = cur["kps"][i1], nb["kps"][i2]
    ur1 = -1.0 if cur["uright"] is None else float(cur["uright"][i1]); ur2 = -1.0 if nb["uright"] is None else float(nb["uright"][i2])
    s1, s2 = ur1 >= 0, ur2 >= 0
    xn1 = np.array([(kp1["x"] - cx1) / fx1, (kp1["y"] - cy1) / fy1, 1.0]); xn2 = np.array([(kp2["x"] - cx2) / fx2, (kp2["y"] - cy2) / fy2, 1.0])
    r1, r2 = R1.T @ xn1, R2.T @ xn2
    cr = r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2))
    c1 = c2 = cr + 1
    if s1:
        c1 = np.cos(2 * np.arctan2(mb1 / 2, float(cur["depth"][i1])))
    elif s2:
        c2 = np.cos(2 * np.arctan2(mb2 / 2, float(nb["depth"][i2])))
    if cr < min(c1, c2) and cr > 0 and (s1 or s2 or cr < 0.9997):
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        v = np.linalg.svd(A)[2][3]
        X = v[:3] / v[3]
    elif s1 and c1 < c2:
        z = float(cur["depth"][i1]); X = R1.T @ np.array([(kp1["x"] - cx1) * z / fx1, (kp1["y"] - cy1) * z / fy1, z]) + O1
    elif s2 and c2 < c1:
        z = float(nb["depth"][i2]); X = R2.T @ np.array([(kp2["x"] - cx2) * z / fx2, (kp2["y"] - cy2) * z / fy2, z]) + O2
    else:
        return ST["PARALLAX"]
    P1, P2 = R1 @ X + t1, R2 @ X + t2
    if P1[2] <= 0 or P2[2] <= 0:
        return ST["DEPTH"]
    for P, kp, ur, st, cam, sig, code in ((P1, kp1, ur1, s1, (fx1, fy1, cx1, cy1), scene["sg"][kp1["octave"]], "REPROJ1"),
                                          (P2, kp2, ur2, s2, (fx2, fy2, cx2, cy2), scene["sg"][kp2["octave"]], "REPROJ2")):
        u, v_ = cam[0] * P[0] / P[2] + cam[2], cam[1] * P[1] / P[2] + cam[3]
        e = (u - kp["x"]) ** 2 + (v_ - kp["y"]) ** 2
        if not st:
            if e > 5.991 * sig:
                return ST[code]
        elif e + (u - mbf1 / P[2] - ur) ** 2 > 7.8 * sig:        # :471: the current keyframe's mbf on both sides
            return ST[code]
    d1, d2 = np.linalg.norm(X - O1), np.linalg.norm(X - O2)
    if d1 == 0 or d2 == 0:
        return ST["DIST_ZERO"]
    rd, ro, rf = d2 / d1, float(scene["sf"][kp1["octave"]]) / float(scene["sf"][kp2["octave"]]), 1.5 * float(scene["scale_factor"])
    return ST["SCALE"] if rd * rf < ro or rd > ro * rf else ST["CREATED"]


def test_gates_recomputed_in_float64_agree_where_the_gap_is_large(restated):
    checked = 0
    for s, r in restated:
        for k, i in zip(*np.nonzero((r["match12"] >= 0) & (r["gap"] >= 1e-3))):
            assert _status64(s, k, i, r["match12"][k, i]) == r["status"][k, i], (s["name"], k, i, r["gap"][k, i])
            checked += 1
    assert checked > 500


def test_restated_points_are_the_float64_null_vectors(restated):
    """e(x) = |x - x64| / |x64| of the created points that came out of the SVD: float accuracy times the triangulation's
    conditioning -- below 1e-3 on these scenes (parallax well above the thresholds)."""
    worst = 0.0
    for s, r in restated:
        for k, i in zip(*np.nonzero((r["status"] == ST["CREATED"]) & r["from_svd"])):
            x64 = cpo.null_vector_f64(r["A"][k, i])
            worst = max(worst, np.linalg.norm(r["x3d"][k, i] - x64) / np.linalg.norm(x64))
    print("restatement: largest e(x) =", worst)
    assert worst < 1e-3


def test_scenes_keep_near_threshold_pairs_under_the_cap(restated):
    """At most 2 % of a scene's matched pairs have a gate gap under 1e-3 in the restatement alone: the device test may then exclude
    pairs under any m <= 1e-3 and stay inside its cap of 2 %."""
    extra = [(s, cpo.create_new_map_points(s)) for s in (scenes.random_scene(400, 2000, 10),)]
    for s, r in list(restated) + extra:
        pairs = r["match12"] >= 0
        low = int((r["gap"][pairs] < 1e-3).sum())
        print(s["name"], "pairs", int(pairs.sum()), "gap < 1e-3:", low)
        assert low <= 0.02 * pairs.sum(), s["name"]


def test_planted_statuses():
    s, expect = scenes.planted_scene()
    r = cpo.create_new_map_points(s)
    inv = {v: k for k, v in ST.items()}
    for name, (k, status) in expect.items():
        i = s["P"][name]
        assert inv[int(r["status"][k, i])] == status, name
        if status == "CREATED":
            assert np.allclose(r["x3d"][k, i], s["X"][i], rtol=0, atol=1e-4), name
    i = s["P"]["coupled"]
    assert r["status"][1, i] == ST["SKIPPED"] and r["match12"][1, i] == -1
    alone = dict(s, neigh=[s["neigh"][1]])
    ra = cpo.create_new_map_points(alone)
    assert ra["status"][0, i] == ST["CREATED"]                      # ... which neighbour 1 would have created
    for name in ("fallback1", "fallback2"):
        assert not r["from_svd"][3, s["P"][name]]                  # UnprojectStereo, not the SVD
    assert r["from_svd"][0, s["P"]["created"]]
    assert set(np.unique(r["status"])) >= {ST[c] for c in ("NO_MATCH", "CREATED", "SKIPPED", "PARALLAX", "DEPTH", "REPROJ1", "REPROJ2", "SCALE")}
    assert r["nnew"] == 5 and np.array_equal(r["counts"].sum(0)[[0, 3, 4, 5, 6, 8]], [5, 1, 1, 1, 2, 1])


# ------------------------------------------------------------------------------------------------ the ABI surface
NEW = ("orbm_create_new_map_points", "orbm_debug_last_create_points_waits")


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def test_new_entry_points_are_declared_and_exported(so):
    protos = _lib.prototypes()
    vp = C.c_void_p
    assert protos["orbm_create_new_map_points"] == (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, vp, vp, vp, vp, vp])
    assert protos["orbm_debug_last_create_points_waits"] == (C.c_int, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    for name in NEW:
        assert f" T {name}\n" in out
    assert _lib.lib().orbx_abi_version() == 136


def test_struct_mirror_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_create_points")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_create_points.c"), "-o", exe])
    fields, enums, size = [], {}, None
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            size = int(w[2])
        elif w[0] == "field":
            fields.append((w[2], int(w[3]), int(w[4])))
        else:
            enums[w[1]] = int(w[2])
    m = _CTriangKeyFrame
    assert C.sizeof(m) == size
    assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields
    for name, v in enums.items():
        assert getattr(ORBmatcher, name.replace("ORBM_", "")) == v == (cpo.STATUS.get(name.replace("ORBM_TRI_", ""), cpo.NSTATUS)), name


def test_refusals_before_the_launch(so):
    """null pointers, K out of range and a bad level count are refused before anything touches a device (a keyframe's octave range
    belongs to its resident frame, which only a device can make: tests/test_gpu_create_points.py has that refusal)"""
    L = _lib.lib()
    kf = _CTriangKeyFrame()                       # every pointer NULL
    arr = (_CTriangKeyFrame * 33)()
    sf = np.ones(8, np.float32); nnew = C.c_int(-5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda cur, ne, K, s=sf, g=sf, nl=8, nn=C.byref(nnew): L.orbm_create_new_map_points(cur, ne, K, p(s) if s is not None else None,
                                                                                           p(g) if g is not None else None, nl, 1.2, None, None,
                                                                                           None, None, nn)
    ERR_ARG, ERR_UNSUPPORTED = -1, -5
    assert call(C.byref(kf), arr, 33) == ERR_UNSUPPORTED
    assert b"32" in L.orbx_last_error()
    assert call(C.byref(kf), arr, -1) == ERR_ARG
    assert call(None, arr, 1) == ERR_ARG
    assert call(C.byref(kf), None, 1) == ERR_ARG
    assert call(C.byref(kf), arr, 1, s=None) == ERR_ARG
    assert call(C.byref(kf), arr, 1, g=None) == ERR_ARG
    assert call(C.byref(kf), arr, 1, nl=0) == ERR_ARG
    assert call(C.byref(kf), arr, 1, nn=None) == ERR_ARG
    assert call(C.byref(kf), arr, 0) == ERR_ARG                     # a current keyframe without a frame
    assert nnew.value == -5                                         # refused calls write nothing
    assert L.orbm_debug_last_create_points_waits() == 0


def test_integration_shell_calls_the_declared_entry_point():
    """integration/LocalMapping_create_hip.cc cannot be compiled here (no OpenCV / DBoW2): its library calls have the declared
    numbers of arguments and every ORBM_ / ORBX_ constant it names exists."""
    import re

    import test_cpu_integration_shells as shells
    decl, header_text = shells._declarations()
    src = open(os.path.join(ROOT, "integration", "LocalMapping_create_hip.cc")).read()
    calls = [c for c in shells._calls(src) if c[0] in decl]
    assert sorted(calls) == [("orbm_create_new_map_points", 12), ("orbx_last_error", 0)] and all(decl[f] == n for f, n in calls)
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", shells._strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    assert "LocalMapping_create_hip.cc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
