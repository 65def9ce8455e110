"""The CPU restatement of Optimizer::PoseOptimization (tests/pose_only_oracle.c) from first principles, and the new C-ABI's
surface without a device: declared, exported, the integration shell calls it correctly, and every entry point refuses to run on
the host (ORBX_ERR_NO_DEVICE: there is no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_only_oracle as po
import pose_only_scene as ps
import pose_optimum as pm
from test_cpu_integration_shells import _declarations, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max()


@pytest.mark.parametrize("stereo", [False, True])
def test_noise_free_scene_recovers_the_true_pose(stereo):
    p = ps.noise_free(1 + stereo, 200, stereo)
    ng, T, out, st = po.run(p)
    assert ng == 200 and not out.any() and st.rounds == 4
    q = po.quat_from_matrix(p["Rt"])
    assert _rel(st.q, q) < 1e-9
    # the stereo edge's cam_project rounds invz to float: its third error component is flat below the float resolution of
    # 1 / z, so the depth of the optimum is pinned only to that (a few 1e-9 here)
    assert _rel(st.t, p["tt"]) < (5e-9 if stereo else 1e-9)
    R0 = p["Tcw"][:3, :3].astype(np.float64)
    assert np.degrees(np.arccos(np.clip((np.trace(R0 @ p["Rt"].T) - 1) / 2, -1, 1))) > 1.0      # the start was degrees off
    assert np.linalg.norm(p["Tcw"][:3, 3] - p["tt"]) > 0.01


@pytest.mark.parametrize("stereo", [False, True])
def test_jacobians_match_central_differences(stereo):
    rng = np.random.default_rng(5)
    cam = ps.CAM
    for _ in range(20):
        T = po.se3_from_cv(ps.pose44(ps.rodrigues(rng.normal(0, 0.5, 3)), rng.normal(0, 0.3, 3)))
        Xw = np.array([*rng.uniform(-1, 1, 2), 0.0]) + np.array([0, 0, 3.0])
        R = po.quat_to_matrix(T.q)
        Xw = R.T @ (np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)]) - np.array(T.t))
        obs = np.array([300.0, 200.0, 280.0])
        J = po.edge_jacobian(cam, stereo, Xw, T)
        h = 1e-6 if not stereo else 1e-4       # the stereo error's float invz needs a wider step
        num = np.zeros_like(J)
        for d in range(6):
            u = np.zeros(6)
            u[d] = h
            ep = po.edge_error(cam, stereo, obs, Xw, po.se3_compose(po.se3_exp(u), T))
            u[d] = -h
            em = po.edge_error(cam, stereo, obs, Xw, po.se3_compose(po.se3_exp(u), T))
            num[:, d] = (ep - em) / (2 * h)
        assert np.abs(J - num).max() < 1e-4 * max(1.0, np.abs(J).max()), (J, num)


def test_quaternion_matrix_round_trip():
    rng = np.random.default_rng(7)
    for _ in range(200):
        q = rng.normal(0, 1, 4)
        q /= np.linalg.norm(q)
        q *= np.sign(q[3])
        R = po.quat_to_matrix(q)
        assert _rel(R @ R.T, np.eye(3)) < 1e-14
        q2 = po.quat_from_matrix(R)          # Quaterniond(Matrix3d) may give -q; normalizeRotation makes w >= 0
        assert _rel(q2 * np.sign(q2[3]), q) < 1e-12
    # every branch of Quaterniond(Matrix3d): trace <= 0 with each diagonal entry the largest
    for axis in range(3):
        w = np.zeros(3)
        w[axis] = np.pi * 0.9
        R = ps.rodrigues(w)
        q = po.quat_from_matrix(R)
        assert _rel(po.quat_to_matrix(q), R) < 1e-14


def test_ldlt_matches_numpy_and_refuses_indefinite():
    rng = np.random.default_rng(9)
    for _ in range(100):
        A = rng.normal(0, 1, (6, 6))
        H = A @ A.T + 1e-3 * np.eye(6)
        b = rng.normal(0, 1, 6)
        x = po.ldlt_solve(H, b)
        assert x is not None and _rel(x, np.linalg.solve(H, b)) < 1e-8 * max(1, np.abs(x).max())
    for _ in range(50):
        A = rng.normal(0, 1, (6, 6))
        H = A @ np.diag([3, 2, 1, 1, -1, 2.0]) @ A.T
        assert po.ldlt_solve(H, rng.normal(0, 1, 6)) is None
    # a zero matrix has ZeroSign: isPositive() holds and the solution is 0
    assert np.array_equal(po.ldlt_solve(np.zeros((6, 6)), np.ones(6)), np.zeros(6))


@pytest.mark.parametrize("stereo_frac", [0.0, 0.5])
def test_injected_gross_outliers_end_flagged(stereo_frac):
    p = ps.make_problem(3, 500, stereo_frac=stereo_frac, outlier_frac=0.2, noise_px=0.3)
    ng, T, out, st = po.run(p)
    bad = p["bad"]
    assert bad.sum() > 50 and out[bad].all()
    assert ng == int(p["has_mp"].sum()) - int(out[p["has_mp"] > 0].sum())
    assert np.abs(T[:3, 3] - p["tt"]).max() < 0.01


def test_fewer_than_three_correspondences():
    p = ps.make_problem(4, 30, fill=0.0)
    p["has_mp"][[2, 9]] = 1
    ng, T, out, st = po.run(p, outlier_in=np.ones(30, np.uint8))
    assert ng == 0 and st.rounds == 0 and st.ninitial == 2
    assert np.array_equal(T, p["Tcw"])
    assert out[2] == 0 and out[9] == 0 and out.sum() == 28       # mvbOutlier reset where a map point is, untouched elsewhere


def test_fewer_than_ten_edges_run_one_round():
    for n, rounds in ((9, 1), (10, 4), (3, 1)):
        p = ps.make_problem(5, n, fill=1.0)
        ng, T, out, st = po.run(p)
        assert st.rounds == rounds and st.ninitial == n
        assert all(st.iterations[i] == 0 for i in range(rounds, 4))


def test_round_four_is_not_robustified():
    """The Huber kernel goes after the classification of round 3: round 4's chi2 is the plain sum, rounds 1-3 the Huber sum."""
    seen = 0
    for seed in range(40):
        p = ps.make_problem(seed, 200, stereo_frac=0.3, outlier_frac=0.1, noise_px=1.2)
        ng, T, out, st = po.run(p)
        for r in range(3):
            assert st.round_chi2[r] == st.chi2_robust[r]
        assert st.round_chi2[3] == st.chi2_plain[3] == st.chi2
        seen += st.chi2_plain[3] != st.chi2_robust[3]
    assert seen > 0          # some scenes do have active edges above the Huber threshold in round 4


# ------------------------------------------------------------------------------------------------ the C-ABI without a device

NAMES = ("orbm_pose_optimization", "orbm_frame_pose_optimization", "orbm_pose_optimization_batch")


def _lib():
    from orb_slam2_e_amd._lib import lib
    return lib()


def test_new_symbols_declared_and_exported():
    decl, _ = _declarations()
    lib = _lib()
    assert decl["orbm_pose_optimization"] == 11 and decl["orbm_frame_pose_optimization"] == 9
    assert decl["orbm_pose_optimization_batch"] == 14
    for n in NAMES:
        assert hasattr(lib, n)
    assert lib.orbx_abi_version() == 136


def test_pose_shell_calls_only_declared_entry_points():
    """integration/Optimizer_pose_hip.cc: every C-ABI call is declared with that many arguments and exported; every type and
    constant it names exists (the checks test_cpu_integration_shells.py applies to the other shells)."""
    decl, header = _declarations()
    lib = _lib()
    src = _strip_comments(open(os.path.join(ROOT, "integration", "Optimizer_pose_hip.cc")).read())
    calls = 0
    for m in re.finditer(r"\b((?:orbx|orbm|fem)_[a-z0-9_]+)\s*\(", src):
        i = m.end(); depth = 1; nargs = 0; seen = False
        while depth:
            c = src[i]
            if c in "([{": depth += 1
            elif c in ")]}": depth -= 1
            elif c == "," and depth == 1: nargs += 1
            elif not c.isspace(): seen = True
            i += 1
        fn = m.group(1)
        if fn not in decl:
            assert re.search(r"\b%s\b" % fn, header), fn
            continue
        assert decl[fn] == (nargs + 1 if seen else 0), fn
        assert hasattr(lib, fn)
        calls += 1
    for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert re.search(r"\b%s\b" % tok, header), tok
    assert calls >= 2 and "orbm_pose_optimization" in src and "orbm_frame_pose_optimization" in src
    assert "HipPoseOptimization" in src and "SetPose" in src and "mvbOutlier" in src


def test_python_entry_points_without_a_device():
    """Without a device every entry point returns ORBX_ERR_NO_DEVICE (no CPU fallback); with one, the same calls succeed."""
    import torch
    from orb_slam2_e_amd import OrbxError, pose_optimization, pose_optimization_batch
    p = ps.make_problem(1, 50)
    calls = [lambda: pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"], p["Tcw"]),
             lambda: pose_optimization_batch([p, p], ps.CAM, ps.inv_level_sigma2())]
    for call in calls:
        if torch.cuda.is_available():
            call()
            continue
        with pytest.raises(OrbxError) as e:
            call()
        assert e.value.code == -2


def test_cxx_class_without_a_device(tmp_path):
    """orbslam_hip::PoseOptimization (include/orbslam_hip.hpp) from C++: ORBX_ERR_NO_DEVICE without a device, ORBX_OK with one."""
    import subprocess
    import torch
    from orb_slam2_e_amd._lib import SO_PATH
    _lib()
    src = tmp_path / "pose.cpp"
    src.write_text('#include "orbslam_hip.hpp"\n'
                   "int main() {\n"
                   "    orbslam_hip::PoseOptimization po(500, 500, 320, 240, 40, std::vector<float>(8, 1.f));\n"
                   "    std::vector<orbx_keypoint> k(5);\n"
                   "    for (int i = 0; i < 5; ++i) { k[i].x = 300.f + 10 * i; k[i].y = 200.f + 7 * i * i; }\n"
                   "    std::vector<uint8_t> has(5, 1), out;\n"
                   "    std::vector<float> pos(15);\n"
                   "    for (int i = 0; i < 15; ++i) pos[i] = (i % 3 == 2) ? 4.f : 0.1f * (i % 7) - 0.3f;\n"
                   "    float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};\n"
                   "    const int r = po(k, {}, has, pos, T, out);\n"
                   '    std::printf("%d %d\\n", r, po.status());\n'
                   "}\n")
    exe = tmp_path / "pose"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), SO_PATH,
                           "-Wl,-rpath," + os.path.dirname(SO_PATH), "-o", str(exe)])
    r, status = map(int, subprocess.check_output([str(exe)]).split())
    if torch.cuda.is_available():
        assert status == 0 and r >= 0
    else:
        assert (r, status) == (-1, -2)


# ------------------------------------------------------------------------------------------------ refusals before the device

ERR_ARG, ERR_UNSUPPORTED = -1, -5


def _raw_host_forms(p, inv=None, nlevels=None, off=None):
    """orbm_pose_optimization and orbm_pose_optimization_batch (is_device = 0) through raw ctypes on problem p, with the camera's
    inv_level_sigma2 / nlevels and the batch's kp_off overridable.  Returns their two status codes."""
    from orb_slam2_e_amd.pose import PoseCamera, PoseStats, _kps
    L = _lib()
    n = len(p["has_mp"])
    k = _kps(p["kp_xy"], p["octave"])
    ur = np.ascontiguousarray(p["uright"], np.float32)
    has = np.ascontiguousarray(p["has_mp"], np.uint8)
    mp = np.ascontiguousarray(p["mp_pos"], np.float32)
    invs = np.ascontiguousarray(p["inv_sigma2"], np.float32)
    cam = PoseCamera(*[float(v) for v in p["cam"][:5]], len(invs) if nlevels is None else nlevels,
                     invs.ctypes.data if inv is None else inv)
    Tin = np.ascontiguousarray(p["Tcw"], np.float32)
    Tout = np.zeros(16, np.float32)
    out = np.zeros(max(n, 1), np.uint8)
    ng = np.zeros(2, np.int32)
    st = PoseStats()
    a = ctypes.c_void_p
    r1 = L.orbm_pose_optimization(a(k.ctypes.data), a(ur.ctypes.data), n, a(has.ctypes.data), a(mp.ctypes.data), ctypes.byref(cam),
                                  a(Tin.ctypes.data), a(Tout.ctypes.data), a(out.ctypes.data), a(ng.ctypes.data), ctypes.byref(st))
    off = np.array([0, n] if off is None else off, np.int32)
    B = len(off) - 1
    Tin_b = np.ascontiguousarray(np.tile(Tin.reshape(16), (max(B, 1), 1)))
    Tout_b = np.zeros_like(Tin_b)
    ng_b = np.zeros(max(B, 1), np.int32)
    r2 = L.orbm_pose_optimization_batch(a(k.ctypes.data), a(ur.ctypes.data), a(off.ctypes.data), B, a(has.ctypes.data), a(mp.ctypes.data),
                                        ctypes.byref(cam), a(Tin_b.ctypes.data), a(Tout_b.ctypes.data), a(out.ctypes.data),
                                        a(ng_b.ctypes.data), None, 0, None)
    return r1, r2


def test_host_forms_refuse_before_the_device():
    """Every refusal of the host forms happens before the device is touched, so it is the same with or without one."""
    p = ps.make_problem(60, 8193, stereo_frac=0.5)
    assert _raw_host_forms(p) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    p = ps.make_problem(61, 100, stereo_frac=0.5)
    for nl in (0, 33):
        assert _raw_host_forms(p, nlevels=nl) == (ERR_ARG, ERR_ARG)
    assert _raw_host_forms(p, inv=0) == (ERR_ARG, ERR_ARG)
    assert _raw_host_forms(p, off=[1, 100])[1] == ERR_ARG                      # kp_off[0] != 0
    assert _raw_host_forms(p, off=[0, 60, 40, 100])[1] == ERR_ARG              # decreasing kp_off
    for bad in (-1, 8, 100):                                                   # nlevels = 8
        q = dict(p, octave=p["octave"].copy(), has_mp=p["has_mp"].copy())
        q["has_mp"][37] = 1
        q["octave"][37] = bad
        assert _raw_host_forms(q) == (ERR_ARG, ERR_ARG)
    # a batch of 0 problems is done before anything else is looked at
    assert _raw_host_forms(p, off=[0])[1] == 0


def test_host_forms_accept_a_bad_octave_without_a_map_point():
    """The octave of a keypoint without a map point is never read (no edge): no refusal.  Without a device the call then stops
    at ORBX_ERR_NO_DEVICE, with one it runs."""
    import torch
    p = ps.make_problem(62, 100, stereo_frac=0.5)
    p["has_mp"][[5, 6]] = 0
    p["octave"][5], p["octave"][6] = -3, 40
    expect = 0 if torch.cuda.is_available() else -2
    assert _raw_host_forms(p) == (expect, expect)
    assert _raw_host_forms(p, off=[0, 50, 50, 100])[1] == expect                # with an empty problem in the batch


# ------------------------------------------------------------------------------------------------ the optimality check's calibration

def _fuzz_scenes(count, seed):
    """fuzz_pose.py-style random scenes"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        nk = int(rng.choice([50, 300, 1000, 3000, 8192]))
        yield ps.make_problem(int(rng.integers(1 << 30)), nk, stereo_frac=float(rng.choice([0.0, 0.5, 1.0])),
                              outlier_frac=float(rng.uniform(0, 0.5)), noise_px=float(rng.choice([0.5, 1.0, 2.0])),
                              rot_deg=float(rng.choice([1.0, 5.0, 20.0])), trans_m=float(rng.choice([0.02, 0.1, 0.5])),
                              fill=float(rng.uniform(0.3, 1.0)))


def _round4_check(p):
    ng, T, out, st, edges = po.run(p, edges=True)
    if st.rounds != 4 or st.iterations[3] >= 10:
        return None
    act = pm.round4_active(edges)
    if len(act) < pm.MIN_EDGES:
        return None
    return pm.gauss_newton_check(p, act, st.q, st.t)


def test_optimality_tolerances_hold_on_the_restatement_with_a_10x_margin():
    """tests/pose_optimum.py's STEP_TOL / GAIN_TOL: every scene the device is held to, and 60 random ones, stay 10x inside both
    on the restatement.  The device scenes also keep their preconditions: no classification near its threshold, and round 4
    stopped by Raul's criterion."""
    checked = 0
    for name, (seed, n, sf, of, kw) in sorted(pm.SCENES.items()):
        p = ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=of, **kw)
        st = po.run(p)[3]
        assert st.min_class > 1e-6, name
        r = _round4_check(p)
        assert r is not None, name
        assert r[0] <= pm.STEP_TOL / 10 and r[1] <= pm.GAIN_TOL / 10, (name, r)
        checked += 1
    for p in _fuzz_scenes(60, 17):
        r = _round4_check(p)
        if r is None:
            continue
        assert r[0] <= pm.STEP_TOL / 10 and r[1] <= pm.GAIN_TOL / 10, r
        checked += 1
    assert checked >= 40


def test_optimality_check_sees_a_slightly_wrong_pose():
    """The check has teeth: the restatement's pose moved by 1e-4 rad or 2e-4 m fails it, mono and stereo."""
    for name in ("mono_1000", "stereo_1000", "mixed_300"):
        seed, n, sf, of, kw = pm.SCENES[name]
        p = ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=of, **kw)
        ng, T, out, st, edges = po.run(p, edges=True)
        act = pm.round4_active(edges)
        T0 = pm.pose_matrix(st.q, st.t)
        for d in (np.array([1e-4, 0, 0, 0, 0, 0]), np.array([0, 0, 0, 0, 0, 2e-4])):
            T1 = pm.exp_se3(d) @ T0
            q = po.quat_from_matrix(T1[:3, :3])
            step, gain, _ = pm.gauss_newton_check(p, act, q, T1[:3, 3])
            assert step > pm.STEP_TOL or gain > pm.GAIN_TOL, (name, d, step, gain)


def test_optimality_helper_is_independent_of_the_restatement():
    """pose_optimum's exp map and quaternion matrix against closed forms: a rotation about z by theta, a pure translation."""
    th = 0.3
    T = pm.exp_se3([0, 0, th, 0, 0, 0])
    assert np.abs(T[:3, :3] - ps.rodrigues(np.array([0, 0, th]))).max() < 1e-15
    assert np.abs(pm.exp_se3([0, 0, 0, 1, 2, 3])[:3, 3] - [1, 2, 3]).max() == 0
    q = np.array([0, 0, np.sin(th / 2), np.cos(th / 2)])
    assert np.abs(pm.quat_matrix(q) - ps.rodrigues(np.array([0, 0, th]))).max() < 1e-15


def test_pose_forms_program_compiles(tmp_path):
    """tests/cxx/pose_forms.cpp (both orbslam_hip::PoseOptimization overloads; run by tests/test_gpu_pose_edges.py) builds with g++
    against the library."""
    import subprocess
    from orb_slam2_e_amd._lib import SO_PATH
    _lib()
    exe = tmp_path / "pose_forms"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "pose_forms.cpp"), SO_PATH, "-Wl,-rpath," + os.path.dirname(SO_PATH), "-o", str(exe)])
    assert exe.exists()
