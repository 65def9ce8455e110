"""PoseOptimizationNR's bundle on the device, the part that needs no device: the CPU restatement (tests/pose_nr_bundle_oracle.c) held
to first principles -- a noise-free rigid scene, its Jacobians against central differences, its Schur step against a dense solve --
and to the closed-loop yardstick (oracle/pose_nr_oracle.c over oracle/mini_g2o.h) on the four closed-loop scenes; the margins that
keep every decision of those scenes away from the tolerances; the layout of the new ABI structs; the refusals before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import pose_nr_bundle_oracle as nrb
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import pose as P
from pose_nr_scene import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5

# The closed-loop scenes of tests/test_gpu_fem.py::test_pose_optimization_nr_closed_loop (deform 0.003, 0.5 px noise, pose error
# (0.005, 0.01)).  `large` has seed 5 here, not 2: with seed 2 one ACCEPTED trial of the restatement has
# |currentChi - tempChi| = 6.2e-4 (|currentChi| + |tempChi|), inside the margin this file requires (seed 5: 5.4e-3 at the least).
SCENES = [("min", 1), ("median", 1), ("p90", 2), ("large", 5)]

# Largest differences between the restatement and the yardstick over the four scenes, measured on the CPU (x86-64, gcc -O2, glibc);
# both sides are double on the same machine, so a bound of 10 x the measured value absorbs libm and compiler differences.  No bound
# is looser than the closed-loop test's own (CAP).  Per scene (min, median, p90, large):
#   sE          6.0e-5  6.3e-6  2.5e-6  6.0e-6       nsE         6.0e-5  6.3e-6  2.5e-6  5.9e-6
#   tempChi     1.6e-5  3.3e-6  2.1e-6  4.1e-6       currentChi  8.0e-6  2.1e-6  1.1e-6  2.0e-7
#   lambda      1.6e-5  7.9e-11 2.5e-7  5.7e-9
#   R           9.3e-7  3.0e-8  2.9e-8  2.3e-8       t / extent  7.5e-7  6.7e-10 2.8e-8  1.3e-8      X / extent  8.5e-7  7.7e-9  1.1e-8  7.5e-9
# (`min` has 10 points and 26 edges: its bundle is the least constrained, and what the float Huber threshold and the quaternion
# normalisation change in the last digits of a step grows most there.)
MEASURED = {"sE": 6.0e-5, "nsE": 6.0e-5, "tempChi": 1.6e-5, "currentChi": 8.0e-6, "lam": 1.6e-5, "R": 9.3e-7, "t": 7.5e-7, "X": 8.5e-7}
CAP = {"sE": 1e-4, "nsE": 1e-4, "tempChi": 1e-4, "currentChi": 1e-4, "lam": 1e-4, "R": 1e-6, "t": 1e-6, "X": 1e-6}
BOUND = {k: min(10 * v, CAP.get(k, np.inf)) for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def problems():
    """name -> (top, graph, yardstick scene, K, u0, ids, restatement's result), each computed once"""
    out = {}
    for name, seed in SCENES:
        top, tris, g, sc, K, u0, ids = nrb.fixture_problem(name, seed)
        out[name] = (top, g, sc, K, u0, ids, nrb.pose_optimization_nr(g, K, u0, ids))
    return out


# ------------------------------------------------------------------------------------------------ 1. the restatement from first principles
def test_noise_free_rigid_scene_converges_to_the_true_pose():
    """No deformation, no pixel noise, no outliers, six keyframes, the frame's pose 0.005 rad / 1 % of the extent off, and a stiffness
    matrix of zeros: the hook then adds exactly 0 to every chi2 and the loop is Levenberg on the reprojection error alone, whose
    minimum is the true pose with the map's own points.  (With the real K the reference's weighting -- currentChi += nsE, then
    tempChi = chi2 + 2 nsE on an iteration's first trial and + 5 nsE on its retries -- ends the rounds early: this scene then stops
    8e-5 from the true rotation.  That is the reference's loop and is compared as it is against the yardstick below.)  What is left
    is the rounding of the inputs to float: 3e-5 px in an observation at 517 px focal length is 6e-8 rad, 6e-8 relative in the pose;
    the bound is 1e-6 for the rotation's entries and for the translation over the extent, and the robust chi2 falls below 1e-6 of
    where it started."""
    m = np.load(os.path.join(ROOT, "tests", "golden", "fem_mesh_median.npz"))
    top = m["points"]
    sc = make_scene(top, seed=3, nkf=6, deform=0.0, noise_px=0.0, outlier_frac=0.0, pose_err=(0.005, 0.01))
    g = nrb.graph_from_scene(sc)
    ntop = len(top)
    nodes = oracle.fem_second_layer(top, 0.5)
    ids = np.arange(ntop, 2 * ntop, dtype=np.int32)
    r = nrb.pose_optimization_nr(g, np.zeros((6 * ntop, 6 * ntop), np.float32), nodes.ravel(), ids)
    ext = np.linalg.norm(top.max(0) - top.min(0))
    R0 = g["Tcw"].reshape(4, 4)[:3, :3].astype(np.float64)
    assert np.abs(R0 - sc["Rf"]).max() > 1e-3                                       # it started away from the answer
    assert not r["trials"]["nsE"].any()
    assert np.abs(nrb.quat_to_matrix(r["q"]) - sc["Rf"]).max() <= 1e-6
    assert np.abs(r["t"] - sc["tf"]).max() <= 1e-6 * ext
    assert r["trials"]["currentChi"][-1] <= 1e-6 * r["trials"]["currentChi"][0]
    assert r["ngood"] == len(top) and not r["outlier"].any()


def test_analytic_jacobians_match_central_differences():
    """linearizeOplus (types_six_dof_expmap.cpp:103-147) against (e(x + h) - e(x - h)) / 2h with h = 1e-6: the point by addition, the
    pose by exp(h e_j) * T.  Truncation h^2 |e'''| / 6 and rounding eps |e| / h are both below 1e-6 of the largest entry."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        w = rng.normal(0, 0.3, 3)
        th = np.linalg.norm(w); k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx; T[:3, 3] = rng.normal(0, 0.2, 3)
        est = nrb.se3_from_cv(T)
        Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])          # in front of the camera
        X = nrb.quat_to_matrix(est.q[:]).T @ (Xc - np.array(est.t[:]))
        cam = np.array([517.3, 516.5, 318.6, 255.3], np.float32); obs = rng.uniform(100, 400, 2).astype(np.float32)
        _, A, B = nrb.edge(est, X, obs, cam)
        h = 1e-6
        An = np.zeros((2, 3)); Bn = np.zeros((2, 6))
        for j in range(3):
            d = np.zeros(3); d[j] = h
            An[:, j] = (nrb.edge(est, X + d, obs, cam)[0] - nrb.edge(est, X - d, obs, cam)[0]) / (2 * h)
        for j in range(6):
            d = np.zeros(6); d[j] = h
            Bn[:, j] = (nrb.edge(nrb.oplus_pose(est, d), X, obs, cam)[0] - nrb.edge(nrb.oplus_pose(est, -d), X, obs, cam)[0]) / (2 * h)
        assert np.abs(A - An).max() <= 1e-6 * np.abs(A).max()
        assert np.abs(B - Bn).max() <= 1e-6 * np.abs(B).max()


def test_schur_step_equals_a_dense_solve_of_the_damped_system():
    """5 points, their frame edges and keyframe edges: x of the Schur step against numpy's solve of the full (6 + 15)-dimensional
    (H + lambda I) x = b, to 1e-9 of |x| (both are backward stable on a system whose condition number is about 1e6)."""
    m = np.load(os.path.join(ROOT, "tests", "golden", "fem_mesh_median.npz"))
    sc = make_scene(m["points"][:5], seed=2, deform=0.003, noise_px=0.5, pose_err=(0.005, 0.01), outlier_frac=0.0)
    g = nrb.graph_from_scene(sc)
    ok, Hpp, bp, Hll, bl, Hpl, _ = nrb.first_step(g, 0.0)
    lam = 1e-5 * max(np.abs(np.diag(Hpp)).max(), max(np.abs(np.diag(h)).max() for h in Hll))     # computeLambdaInit
    ok, Hpp, bp, Hll, bl, Hpl, x = nrb.first_step(g, lam)
    assert ok
    n = 5
    H = np.zeros((6 + 3 * n, 6 + 3 * n)); b = np.zeros(6 + 3 * n)
    H[:6, :6] = np.tril(Hpp) + np.tril(Hpp, -1).T; b[:6] = bp
    for i in range(n):
        s = slice(6 + 3 * i, 9 + 3 * i)
        H[s, s] = Hll[i]; H[:6, s] = Hpl[i]; H[s, :6] = Hpl[i].T; b[s] = bl[i]
    ref = np.linalg.solve(H + lam * np.eye(len(b)), b)
    assert np.abs(x).max() > 0 and np.abs(x - ref).max() <= 1e-9 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ 2. the restatement against the yardstick
@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_restatement_matches_the_closed_loop_yardstick(name, problems):
    """oracle.pose_optimization_nr on the same float-valued graph: the accept / reject sequence, qmax, the results per iteration, the
    outlier flags and the inlier count are equal; the continuous quantities differ by what the restatement's g2o-literal pieces
    change, bounded at 10 x the measured differences (MEASURED above) and never looser than the closed-loop test's bounds."""
    top, g, sc, K, u0, ids, r = problems[name]
    ref, rres, rR, rt, rX, rinl, rout = oracle.pose_optimization_nr(sc, K, u0, ids)
    tr = r["trials"]
    assert 20 < len(ref) and 0 < ref["acc"].sum() < len(ref) and ref["qmax"].max() >= 2 and 1 in rres        # accepts, rejects, retries
    assert len(tr) == len(ref) and np.array_equal(r["results"], rres)
    assert np.array_equal(tr["qmax"], ref["qmax"]) and np.array_equal(tr["acc"], ref["acc"])
    assert r["ngood"] == rinl and np.array_equal(r["outlier"], rout)
    ext = np.linalg.norm(top.max(0) - top.min(0))
    got = {f: float(np.max(np.abs(tr[f].astype(np.float64) - ref[f]) / np.abs(ref[f]))) for f in ("sE", "nsE", "tempChi", "currentChi", "lam")}
    got["R"] = float(np.abs(nrb.quat_to_matrix(r["q"]) - rR).max())
    got["t"] = float(np.abs(r["t"] - rt).max() / ext); got["X"] = float(np.abs(r["X"] - rX).max() / ext)
    print(name, {k: f"{v:.2e}" for k, v in got.items()})
    for k, v in got.items():
        assert v <= BOUND[k], (k, v, BOUND[k])
    # the write-back is the float of the estimates
    assert np.array_equal(r["points"], r["X"].astype(np.float32))
    assert np.array_equal(r["Tcw"][:3, :3], nrb.quat_to_matrix(r["q"]).astype(np.float32)) and np.array_equal(r["Tcw"][:3, 3], r["t"].astype(np.float32))


@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_every_decision_of_the_scenes_clears_the_margin(name, problems):
    """|currentChi - tempChi| >= 1e-3 (|currentChi| + |tempChi|) at every trial of the restatement, accepted and rejected (10 x the
    1e-4 the device may differ by), with currentChi as the decision saw it; no classification within 1e-6 relative of 5.991.
    Measured minima (rejected, accepted, classification / 5.991): min 3.9e-3 2.5e-3 0.28; median 1.8e-2 5.9e-3 0.53; p90 0.16 0.11
    0.37; large 5.4e-3 1.6e-2 7.1e-3."""
    r = problems[name][6]
    tr = r["trials"]
    before = tr["tempChi"] + tr["diff"]                     # currentChi when rho was formed (an accepted trial overwrites it)
    ok = np.isfinite(tr["tempChi"]) & (tr["tempChi"] < 1e300)
    m = np.abs(tr["diff"][ok]) / (np.abs(before[ok]) + np.abs(tr["tempChi"][ok]))
    assert m.min() >= 1e-3, m.min()
    assert (tr["acc"] == 1).any() and (tr["acc"] == 0).any()
    assert r["class_margin"].min() >= 1e-6 * 5.991


@pytest.mark.parametrize("name", [s[0] for s in SCENES] + ["hex"])
def test_independent_step_from_the_result_is_calibrated_on_the_restatement(name, problems):
    """tests/pose_nr_optimum.py on the restatement's results: (a) the cost at the result is the last accepted trial's tempChi, (b) one
    damped Gauss-Newton step from the result (numpy, central-difference Jacobians, dense solve) reproduces the tempChi of the trial
    that followed.  Both must lie 10 x inside the bound the device is held to (tests/test_gpu_pose_nr.py).  Measured (a) / (b):
    min 3.3e-8 / 9.3e-8, median 4.8e-8 / 1.7e-8, p90 1.2e-7 / 6.3e-8, large 1.2e-7 / 3.8e-8, C3D8 with derived nodes 3.0e-7 / 7.0e-9;
    the pose part of the step is 9e-4 .. 4e-2: the result is NOT a stationary point, which is why the step is compared with the
    trial the loop itself made and not with zero."""
    import pose_nr_optimum as po
    if name == "hex":
        top, quads, der, g, _, K, u0, ids = nrb.hex_problem("median", 5, 12)
        r = nrb.pose_optimization_nr(g, K, u0, ids, der)
    else:
        top, g, _, K, u0, ids, r = problems[name]
        der = None
    a, b, step = po.check(po.Problem(g, K, u0, ids, der), r["q"], r["t"], r["X"], r["trials"], r["trials_per_round"], r["levels"])
    print(name, f"{a:.2e} {b:.2e} {step:.2e}")
    assert b is not None and a <= po.TOL / 10 and b <= po.TOL / 10
    # and the check can fail: the same step from a result 1e-4 of the extent away does not land on the logged trial
    ext = np.linalg.norm(top.max(0) - top.min(0))
    _, b_off, _ = po.check(po.Problem(g, K, u0, ids, der), r["q"], r["t"] + 1e-4 * ext, r["X"], r["trials"], r["trials_per_round"], r["levels"])
    assert b_off > po.TOL


# ------------------------------------------------------------------------------------------------ 3. the ABI
def test_python_mirrors_have_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_pose_nr")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_pose_nr.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    for m, name in ((P.PoseNRGraph, "orbm_pose_nr_graph"), (P.PoseNRResult, "orbm_pose_nr_result"), (P.PoseNRStats, "orbm_pose_nr_stats")):
        assert C.sizeof(m) == sizes[name]
        assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name]
    d = P.NR_TRIAL_DTYPE
    assert d.itemsize == sizes["orbm_pose_nr_trial"] == nrb.TRIAL_DTYPE.fields["diff"][1]
    assert [(d.fields[n][1], d.fields[n][0].itemsize) for n in d.names] == [(o, w) for _, o, w in fields["orbm_pose_nr_trial"]]


# ------------------------------------------------------------------------------------------------ 4. refusals before any launch
def _graph(n=4, nkf=2, edges=((0, -1), (0, 1), (1, -1), (2, -1), (3, -1), (3, 0))):
    e = np.array(edges, np.int32).reshape(-1, 2)
    ne = len(e)
    return {"Tcw": np.eye(4, dtype=np.float32).reshape(16), "kf_Tcw": np.tile(np.eye(4, dtype=np.float32).reshape(16), (nkf, 1)),
            "points": np.tile(np.array([0.1, 0.2, 3.0], np.float32), (n, 1)) * (1 + np.arange(n, dtype=np.float32)[:, None]), "e_point": e[:, 0].copy(),
            "e_cam": e[:, 1].copy(), "e_obs": np.full((ne, 2), 300, np.float32), "e_inv_sigma2": np.ones(ne, np.float32),
            "e_cam_k": np.tile(np.array([500, 500, 320, 240], np.float32), (ne, 1))}


def _rc(graph, sizes=None):
    g = P._nr_graph(graph)
    for k, v in (sizes or {}).items():
        setattr(g, k, v)
    res, pts, outlier, _, _, _ = P._nr_buffers(max(len(graph["points"]), 1), False)
    return _lib.lib().orbm_pose_optimization_nr(None, C.byref(g), C.byref(res), None)


def test_refusals_need_no_device():
    """The graph is checked before the model and before the device: limits give ORBX_ERR_UNSUPPORTED, a malformed graph and a missing
    model ORBX_ERR_ARG.  (A model that exists but has had no fem_trial_setup needs a device to be created:
    tests/test_gpu_pose_nr.py.)"""
    assert _rc(_graph(), {"npoints": 1366}) == ERR_UNSUPPORTED
    assert _rc(_graph(), {"nedges": 65537}) == ERR_UNSUPPORTED
    assert _rc(_graph(), {"nkf": 1025}) == ERR_UNSUPPORTED
    assert _rc(_graph(), {"npoints": -1}) == ERR_ARG
    assert _rc(_graph(edges=((0, -1), (2, -1), (1, -1), (3, -1)))) == ERR_ARG          # not grouped by ascending point
    assert _rc(_graph(edges=((0, -1), (1, -1), (4, -1)))) == ERR_ARG                   # point index out of range
    assert _rc(_graph(edges=((0, -1), (1, 2), (3, -1)))) == ERR_ARG                    # keyframe index out of range
    assert _rc(_graph(edges=((0, -1), (1, -2), (3, -1)))) == ERR_ARG
    assert _rc(_graph()) == ERR_ARG                                                    # a well-formed graph without a model
    assert b"fem_trial_setup" in _lib.lib().orbx_last_error()
    L = _lib.lib()
    assert L.orbm_pose_optimization_nr_batch(None, None, -1, None, None) == ERR_ARG
    assert L.orbm_pose_optimization_nr_batch(None, None, 0, None, None) == OK


def test_fewer_than_three_points_return_the_inputs_without_model_or_device():
    """Optimizer.cc:711-714: nInitialCorrespondences < 3 returns 0 before fea2.Compute: the pose and the points stand."""
    g = _graph(n=2, edges=((0, -1), (1, -1), (1, 0)))
    g["Tcw"][3] = 0.25
    ngood, Tcw, pts, outlier, st = P.pose_optimization_nr(None, g, want_stats=True)
    assert ngood == 0 and np.array_equal(Tcw.reshape(16), g["Tcw"]) and np.array_equal(pts, g["points"]) and not outlier.any()
    assert st["ntrials"] == 0 and len(st["results"]) == 0 and np.array_equal(st["X"], g["points"].astype(np.float64))


# ------------------------------------------------------------------------------------------------ 5. the integration shell
def test_integration_shell_calls_declared_entry_points_and_fills_every_field():
    """integration/Optimizer_pose_nr_hip.cc cannot be compiled here (no OpenCV / g2o): its C-ABI calls are declared with that many
    arguments and exported, it sets every member of the graph and of the result, a keyframe edge takes the FRAME keypoint's octave,
    and it says what it does with the mnId == 0 keyframe."""
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, header_text = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_pose_nr_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert ("orbm_pose_optimization_nr", 4) in calls
    for fn, n in calls:
        assert decl[fn] == n and hasattr(_lib.lib(), fn), fn
    for f, _ in P.PoseNRGraph._fields_:
        assert f"g.{f} =" in src, f
    for f in ("points_out", "outlier"):
        assert f"res.{f} =" in src, f
    assert "mvInvLevelSigma2[kpUn.octave]" in src.split("GetKeyPointUn")[1]
    assert "mnId == 0" in raw and "left out" in raw
    for tok in set(__import__("re").findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert tok in header_text, tok
