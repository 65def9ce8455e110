"""OptimizeSim3 on the device, the part that needs no device: the CPU restatement (tests/sim3_opt_oracle.c) held to first principles
-- planted similarities, an analytic Gauss-Newton step in numpy (tests/sim3_optimum.py), Sim3(update) against scipy's expm --, every
quirk of the reference's code path planted once, the sensitivity of the restatement to the last bit of sin / cos / exp (pinned in
tests/golden/sim3_opt_sensitivity.json; tests/test_gpu_sim3_opt.py takes its tolerance from there), and the surfaces: ABI layout,
the C++ smoke program, the integration shell's calls, the refusals before any launch."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_opt_oracle as so
import sim3_opt_scenes as scenes
import sim3_optimum as sm
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import sim3 as s3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_opt_sensitivity.json")
ISG = scenes.INV_SIGMA2
OK, ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -5
ULP_SEEDS = [7919 * k for k in range(1, 17)]
M = 8                    # the project's margin: M = 8 D
CAP = 0.02               # the project's cap on what may lie at the rounding floor


def _ints(r):
    return (r.nin, r.nbad, r.ncorrespondences, tuple(r.iterations), tuple(r.trials))


# ------------------------------------------------------------------------------------------------ 1. the restatement from first principles
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("n", [20, 100])
def test_noise_free_scene_recovers_the_planted_similarity(n, fixed):
    """from 5 degrees / 5 % / 5 % off, to 1e-6 (the observations are floats: about 3e-5 px of rounding)"""
    p = scenes.problem(7, n, noise=0.0, outliers=0.0, fix_scale=fixed)
    o = so.optimize(p, ISG)
    r = o["res"]
    assert r.nin == n and r.nbad == 0 and o["kept"].all()
    assert np.abs(sm.quat_matrix(r.q) - p["R"]).max() < 1e-6
    assert np.abs(np.array(r.t) - p["t"]).max() < 1e-6
    assert abs(r.s - p["s"]) < 1e-6


def test_restatement_ends_at_the_optimum_of_an_analytic_model():
    """One float64 Gauss-Newton step with ANALYTIC Jacobians (tests/sim3_optimum.py) from the restatement's result, on the pairs the
    second round optimised, is small and buys almost nothing: the bounds are the ones tests/test_gpu_pose_edges.py uses
    (tests/pose_optimum.py: STEP_TOL 1e-4, GAIN_TOL 2e-6), unscaled -- the numeric Jacobian's noise floor, ulp(error) / 2e-9 or
    about 3e-5 on entries of 1e2 .. 1e4, moves the optimum by less than that (largest seen: step 4e-5, gain 8e-7)."""
    worst = [0.0, 0.0]
    ran = 0
    for p in scenes.gpu_scenes():
        o = so.optimize(p, ISG)
        r = o["res"]
        if r.ncorrespondences - r.nbad < 10:
            continue
        active = ~np.isnan(o["cut_chi"][1, :, 0])
        assert int(active.sum()) == r.ncorrespondences - r.nbad
        step, gain, cost = sm.gauss_newton_check(p, ISG, active, r.q, r.t, r.s)
        print(p["name"], "step %.2e gain %.2e" % (step, gain))
        assert step <= sm.STEP_TOL and gain <= sm.GAIN_TOL, (p["name"], step, gain)
        assert abs(cost - r.chi2) <= 1e-3 * cost                  # the cost is the one the second round minimised
        worst = [max(worst[0], step), max(worst[1], gain)]
        ran += 1
    assert ran >= 12


def _similarity(S):
    """[[s R(q), t], [0, 0, 0, 1]] with q taken as it is (g2o does not normalise it)"""
    x, y, z, w = S.q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = S.s * R; T[:3, 3] = list(S.t)
    return T


@pytest.mark.parametrize("sigma", [0.0, 3e-6, 0.3, -0.2])
@pytest.mark.parametrize("theta", [0.0, 4e-6, 0.7, 2.9])
def test_sim3_of_an_update_is_the_exponential(theta, sigma):
    """Sim3(Vector7d) (sim3.h:70-142) against expm of the 4 x 4 generator in each of its four branches (|sigma| < 1e-5 or not,
    theta < 1e-5 or not), to 1e-12 apart from the two first-order shortcuts of the small branches: the small-theta ones set
    R = I + Omega + Omega^2 -- not the exponential's I + Omega + Omega^2 / 2, and not orthogonal -- and take Quaterniond(R) from it
    unnormalised (|q|^2 = 1 - theta^2 / 4), the small-sigma ones set C = 1, which moves t by sigma / 2 of upsilon, and B of the
    small-theta / large-sigma one is not the series' limit."""
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    u = np.concatenate([theta * axis, [0.4, -0.7, 0.2], [sigma]])
    S = so.sim3_exp(u)
    E = sm.exp_sim3(u)
    assert S.s == np.exp(sigma)
    dt = np.abs(np.array(S.t) - E[:3, 3]).max()
    if 0 < abs(sigma) < 1e-5:
        assert 0.1 * abs(sigma) < dt < 2 * abs(sigma)             # C = 1 (and A, B of sigma = 0) for a sigma that is not 0
    elif 0 < theta < 1e-5 and sigma != 0:
        assert dt < 2 * theta ** 2 / abs(sigma) ** 3 < 1e-8       # sim3.h:116: B of that branch lacks the limit's "- 1"; it multiplies Omega^2
    else:
        assert dt < 1e-12
    q2 = float(np.dot(S.q, S.q))
    if theta < 1e-5:
        W = sm._hat(u[:3])
        R1 = np.eye(3) + W + W @ W
        assert np.abs(_similarity(S)[:3, :3] / S.s * (1 / q2) - R1).max() < 1e-10     # R(q) = |q|^2 times a rotation
        assert np.abs(np.exp(sigma) * R1 - E[:3, :3]).max() < 1e-10
        assert abs(q2 - (1 - theta * theta / 4)) < 1e-15
        if theta > 0:
            assert q2 < 1 - 1e-12                                 # measurably not a unit quaternion
    else:
        assert abs(q2 - 1) < 1e-14
        assert np.abs(_similarity(S)[:3, :3] - E[:3, :3]).max() < 1e-12


def test_inverse_and_product_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(20):
        A = so.sim3_exp(np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 1.0, 3), rng.normal(0, 0.3, 1)]))
        B = so.sim3_exp(np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 1.0, 3), rng.normal(0, 0.3, 1)]))
        assert np.abs(_similarity(so.mul(A, so.inverse(A))) - np.eye(4)).max() < 1e-12
        assert np.abs(_similarity(so.mul(A, B)) - _similarity(A) @ _similarity(B)).max() < 1e-12
        X = rng.normal(0, 2.0, 3)
        assert np.abs(so.sim3_map(A, X) - (_similarity(A) @ np.append(X, 1))[:3]).max() < 1e-12
        assert np.abs(so.sim3_map(so.inverse(A), so.sim3_map(A, X)) - X).max() < 1e-12


def test_start_is_the_sim3_of_the_float_inputs():
    """Sim3(Matrix3d, Vector3d, double) from the floats LoopClosing.cc:320-325 hands over: Quaterniond(R) of the widened matrix"""
    p = scenes.problem(5, 12)
    S = so.from_rts(p["R12"], p["t12"], p["s12"])
    assert np.abs(sm.quat_matrix(S.q) - p["R12"].astype(np.float64)).max() < 1e-7
    assert list(S.t) == [float(v) for v in p["t12"]] and S.s == float(p["s12"])


def test_ldlt_solves_and_reports_the_sign():
    rng = np.random.default_rng(4)
    A = rng.normal(size=(7, 7)); H = A @ A.T + 0.1 * np.eye(7); b = rng.normal(size=7)
    ok, x = so.ldlt7(np.tril(H), b)                               # only the lower triangle is read
    assert ok and np.abs(x - np.linalg.solve(H, b)).max() < 1e-10
    H[6, :] = 0; H[:, 6] = 0; H[6, 6] = 1e-3; b[6] = 0           # the fixed-scale system: a zero row / column plus lambda
    ok, x = so.ldlt7(H, b)
    assert ok and x[6] == 0 and np.abs(x[:6] - np.linalg.solve(H[:6, :6], b[:6])).max() < 1e-10
    assert not so.ldlt7(-np.eye(7), b)[0] and not so.ldlt7(np.diag([1.0, 1, 1, -1, 1, 1, 1]), b)[0]
    assert so.ldlt7(np.zeros((7, 7)), b) == (True, pytest.approx(np.zeros(7)))
    assert np.isnan(so.ldlt7(np.full((7, 7), np.nan), np.full(7, np.nan))[1][:6]).all()     # Eigen's zero-diagonal exit: NaN in, NaN out


# ------------------------------------------------------------------------------------------------ 2. every quirk, planted once
def test_fixed_scale_gives_an_exact_zero_column_and_an_unchanged_scale():
    p = scenes.problem(9, 40, fix_scale=True)
    P1, P2 = so.prepare(p)
    est = so.from_rts(p["R12"], p["t12"], p["s12"])
    for fixed in (True, False):
        J12, J21 = so.linearize(est, fixed, P1[3], P2[3], p["obs1"][3], p["obs2"][3], p["cam1"], p["cam2"])
        assert np.abs(J12[:, :6]).max(axis=0).min() > 1 and np.abs(J21[:, :6]).max(axis=0).min() > 1
        assert (np.all(J12[:, 6] == 0) and np.all(J21[:, 6] == 0)) == fixed
    o = so.optimize(p, ISG)
    assert o["trace"].H6max == 0.0 and o["trace"].b6 == 0.0      # H(6, .) and b[6]: computeLambdaInit and the LDLT see that zero row
    assert o["res"].s == float(p["s12"]) == 1.0 and o["res"].nin >= 10
    q = dict(p, fix_scale=0)
    assert so.optimize(q, ISG)["trace"].H6max > 0


def test_numeric_jacobian_is_the_central_difference_of_g2o():
    """delta = 1e-9: the columns agree with the analytic Jacobian to the difference's noise floor, ulp(error) / 2e-9"""
    p = scenes.problem(9, 40)
    P1, P2 = so.prepare(p)
    est = so.from_rts(p["R12"], p["t12"], p["s12"])
    E = sm.Pairs(p, ISG, np.ones(p["n"], bool))
    J = E.jacobians(sm.sim3_matrix(est.q, est.t, est.s))
    for i in (0, 17, 39):
        J12, J21 = so.linearize(est, False, P1[i], P2[i], p["obs1"][i], p["obs2"][i], p["cam1"], p["cam2"])
        for num, ana in ((J12, J[i]), (J21, J[p["n"] + i])):
            assert np.abs(num - ana).max() < 1e-3 * max(1.0, np.abs(ana).max())


def test_cut_reads_the_error_of_the_last_tried_estimate():
    """e->chi2() at :1577 / :1611 is the error of the last TRIED estimate: pop() restores the vertex, not the errors."""
    # A pair whose chi2 is on the other side of th2 only at the tried estimate.  Where the last trial of a round is rejected on
    # ordinary data, lambda has grown so far that the tried estimate is the accepted one bit for bit; the case that shows is the NaN
    # one: with a NaN map point every sum is NaN, the
    # update is NaN, the trial is rejected and the estimate stays -- where the pairs' chi2 is far above th2 (the start is 5 degrees
    # off) -- but the cut reads the NaN errors of the tried estimate, and NaN is not > th2: every pair stays
    p = scenes.nan_position()
    o = so.optimize(p, ISG)
    at_start = so.pair_chi2(p, ISG, so.from_rts(p["R12"], p["t12"], p["s12"]))
    assert (np.nanmax(at_start, axis=1) > float(p["th2"])).sum() >= p["n"] - 1
    assert list(o["trace"].eval_is_est) == [0, 0] and np.isnan(o["est"][2].vec()[:7]).all()
    assert np.isnan(o["cut_chi"][0]).all() and o["kept"].all() and o["res"].nbad == 0


def test_iterations_allowed_in_the_second_round():
    """nMoreIterations: 10 if any pair was cut, else 5"""
    cut = so.optimize(scenes.exact(), ISG)
    assert cut["res"].nbad == 3 and cut["res"].iterations[1] == 10 and cut["trace"].hit_limit[1] == 1
    none = so.optimize(scenes.problem(521, 12, noise=0.5, outliers=0.0, off_deg=30.0, off=0.4, th2=1e6), ISG)
    assert none["res"].nbad == 0 and none["res"].iterations[1] == 5 and none["trace"].hit_limit[1] == 1     # still gaining when it ran out


def test_fewer_than_ten_survivors_return_zero_with_the_cut_applied():
    """:1595: nCorrespondences - nBad < 10 returns 0 and leaves g2oS12 as it came in; vpMatches1 already has the cut"""
    p = scenes.problem(200, 10, fix_scale=True, outliers=0.2)
    o = so.optimize(p, ISG)
    r = o["res"]
    assert r.ncorrespondences == 10 and r.nbad == 2 and r.nin == 0 and tuple(r.iterations) == (5, 0)
    assert np.array_equal(o["kept"], ~(o["cut_chi"][0] > float(p["th2"])).any(axis=1)) and int((~o["kept"]).sum()) == 2
    assert np.array_equal(r.vec(), so.from_rts(p["R12"], p["t12"], p["s12"]).vec())                  # bit for bit
    assert not np.array_equal(o["est"][1].vec(), r.vec())                                            # though the first round moved it
    ten = so.optimize(scenes.problem(203, 10, outliers=0.0), ISG)["res"]                             # exactly 10 survivors: on
    assert ten.nbad == 0 and ten.nin == 10 and ten.iterations[1] > 0


@pytest.mark.parametrize("n", range(1, 10))
def test_one_to_nine_pairs_are_still_optimised_and_cut(n):
    p = scenes.problem(40 + n, n, outliers=0.5)
    o = so.optimize(p, ISG)
    r = o["res"]
    assert tuple(r.iterations) == (5, 0) and r.nin == 0 and r.nbad == int((~o["kept"]).sum())
    assert np.array_equal(o["kept"], ~(o["cut_chi"][0] > float(p["th2"])).any(axis=1))
    assert np.array_equal(r.vec(), so.from_rts(p["R12"], p["t12"], p["s12"]).vec())
    assert not np.array_equal(o["est"][1].vec(), r.vec())


def test_some_small_problem_has_a_pair_cut():
    assert sum(so.optimize(scenes.problem(40 + n, n, outliers=0.5), ISG)["res"].nbad for n in range(1, 10)) > 10


def test_nan_position_is_kept_and_counted():
    """A NaN chi2 is not > th2; in Levenberg a NaN rho ends the trial loop after one trial and resets _nBad: 5 + 5 iterations of one
    trial each, no pair cut, nIn = n, the estimate where it started."""
    p = scenes.nan_position()
    o = so.optimize(p, ISG)
    r = o["res"]
    assert _ints(r) == (p["n"], 0, p["n"], (5, 5), (5, 5)) and o["kept"].all() and np.isnan(r.chi2)
    assert np.array_equal(r.vec(), so.from_rts(p["R12"], p["t12"], p["s12"]).vec())


def test_all_outliers_and_no_pair_at_all():
    p = scenes.all_outliers()
    o = so.optimize(p, ISG)
    assert o["res"].nin == 0 and o["res"].nbad > p["n"] - 10 and tuple(o["res"].iterations) == (5, 0)
    p = scenes.problem(1, 0)
    o = so.optimize(p, ISG)
    assert _ints(o["res"]) == (0, 0, 0, (0, 0), (0, 0)) and len(o["kept"]) == 0
    assert np.array_equal(o["res"].vec(), so.from_rts(p["R12"], p["t12"], p["s12"]).vec())


def test_huber_width_is_the_float_square_root():
    """deltaHuber = sqrt(th2) as a float (:1479) and dsqr a float member: th2 = 10 gives delta 3.1622776985168457, not
    3.1622776601683795.  On a scene of gross outliers (every edge in Huber's linear part) the robust chi2 the first round ends
    with is the float one to rounding, and 1e-8 away from the double one."""
    p = scenes.all_outliers()
    o = so.optimize(p, ISG)
    c = so.pair_chi2(p, ISG, o["est"][1]).ravel()
    df = float(np.sqrt(np.float32(10.0)))
    rho = lambda d, dsqr: float(np.sum(np.where(c <= dsqr, c, 2 * np.sqrt(c) * d - dsqr)))
    as_float, as_double = rho(df, float(np.float32(df * df))), rho(np.sqrt(10.0), 10.0)
    assert (c > 10).sum() > p["n"]
    assert abs(as_float - o["res"].chi2) <= 1e-12 * as_float < 1e-3 * abs(as_double - o["res"].chi2)


# ------------------------------------------------------------------------------------------------ 3. sensitivity
def measure_sensitivity():
    """The scenes of the GPU test under the +-1 ulp switch with 16 seeds, on the restatement alone.  D_cpu: the largest relative
    difference of (q, t, s) to the unperturbed run.  Decisions at the rounding floor, counted per scene as DESIGN 10 counts the
    scenes it skips: a kept flag whose chi2 lies within M D_cpu th2 of th2, a trial with |rho| below 1e-9; and, beyond what the
    issue asks, a scene whose integers change under any of the 16 patterns."""
    rows, D = [], 0.0
    for p in scenes.gpu_scenes():
        base = so.optimize(p, ISG)
        v0 = base["res"].vec()
        d, moved = 0.0, 0
        for seed in ULP_SEEDS:
            o = so.optimize(p, ISG, ulp_seed=seed)
            if p["n"]:
                d = max(d, float(np.max(np.abs(o["res"].vec() - v0) / np.abs(v0))))
            moved += _ints(o["res"]) != _ints(base["res"]) or not np.array_equal(o["kept"], base["kept"])
        rows.append(dict(name=p["name"], n=p["n"], fix_scale=p["fix_scale"], d=d, moved=moved, base=base, th2=float(p["th2"])))
        D = max(D, d)
    for r in rows:
        cc = r["base"]["cut_chi"]
        r["near"] = int(np.sum(np.abs(cc[~np.isnan(cc)] - r["th2"]) < M * D * r["th2"]))
        r["small_rho"] = int(r["base"]["trace"].small_rho)
    return D, rows


def test_sensitivity_is_the_pinned_one_and_no_scene_decides_at_the_rounding_floor():
    D, rows = measure_sensitivity()
    floor = [r["name"] for r in rows if r["near"] or r["small_rho"]]
    moved = [r["name"] for r in rows if r["moved"]]
    print("D_cpu %.3e" % D, "scenes at the floor:", floor, "scenes whose integers move:", moved)
    gold = json.load(open(GOLDEN))
    assert gold["scenes"] == [r["name"] for r in rows] and gold["ulp_seeds"] == ULP_SEEDS
    assert len(floor) <= CAP * len(rows), floor               # 21 scenes: none
    assert not moved, moved
    # the pinned figure: the same arithmetic on another libm may round sin / cos / exp differently, which is what D measures
    assert gold["D_cpu"] / 2 <= D <= gold["D_cpu"] * 2, (D, gold["D_cpu"])
    assert 1e-10 < gold["D_cpu"] < 1e-6


# ------------------------------------------------------------------------------------------------ 4. surfaces
@pytest.fixture(scope="module")
def so_path():
    return _lib.build()


def test_new_entry_points_are_declared_exported_and_bound(so_path):
    protos = _lib.prototypes()
    vp = C.c_void_p
    assert protos["orbm_optimize_sim3"] == (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp])
    assert protos["orbm_debug_last_sim3_opt_waits"] == (C.c_int, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for name in ("orbm_optimize_sim3", "orbm_debug_last_sim3_opt_waits"):
        assert f" T {name}\n" in out
    assert _lib.lib().orbx_abi_version() == 136


def test_struct_mirrors_have_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_sim3_opt")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_sim3_opt.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    for m, name in ((s3._CSim3OptProblem, "orbm_sim3_opt_problem"), (s3.Sim3OptResult, "orbm_sim3_opt_result"), (so.Result, "orbm_sim3_opt_result")):
        assert C.sizeof(m) == sizes[name]
        assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name]


def _dev(p):
    return s3.Sim3OptProblem(p["X1w"], p["X2w"], p["obs1"], p["obs2"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"],
                             p["R12"], p["t12"], p["s12"], p["th2"], p["fix_scale"])


def _call(problems, isg=ISG, nlevels=None, P=None):
    L = _lib.lib()
    P = len(problems) if P is None else P
    arr = (s3._CSim3OptProblem * max(len(problems), 1))(*[p.c() for p in problems])
    res = (s3.Sim3OptResult * max(len(problems), 1))()
    kept = np.zeros(max(sum(p.n for p in problems), 1), np.uint8)
    sg = np.ascontiguousarray(isg, np.float32)
    rc = L.orbm_optimize_sim3(arr, P, _lib.ptr(sg), len(sg) if nlevels is None else nlevels, res, _lib.ptr(kept))
    return rc, L.orbm_debug_last_sim3_opt_waits()


def _check_refusals():
    good = _dev(scenes.problem(1, 12))
    assert _call([good] * 65)[0] == ERR_UNSUPPORTED
    assert _call([good], P=-1)[0] == ERR_ARG
    big = scenes.problem(2, 8193)
    assert _call([_dev(big)])[0] == ERR_UNSUPPORTED and b"8,192" in _lib.lib().orbx_last_error()
    assert _call([good, _dev(big)])[0] == ERR_UNSUPPORTED
    # nothing to do: OK, no launch, on any machine
    assert _call([]) == (OK, 0)
    assert _call([_dev(scenes.problem(1, 0)), _dev(scenes.problem(2, 0, fix_scale=True))]) == (OK, 0)
    for field in ("octave1", "octave2"):                                      # an octave outside [0, nlevels)
        for v in (-1, scenes.NLEVELS):
            p = _dev(scenes.problem(1, 12)); getattr(p, field)[7] = v
            assert _call([p])[0] == ERR_ARG and b"octave" in _lib.lib().orbx_last_error()
            assert _call([good, p])[0] == ERR_ARG                            # the second problem of a batch
    assert _call([good], nlevels=0)[0] == ERR_ARG
    assert _lib.lib().orbm_debug_last_sim3_opt_waits() == 0


def test_every_refusal_comes_before_the_launch(so_path):
    import torch
    good = _dev(scenes.problem(1, 12))
    if torch.cuda.is_available():
        assert _call([good]) == (OK, 1)
    else:
        assert _call([good]) == (ERR_NO_DEVICE, 0)                           # valid input, no device: loud
        assert b"no usable HIP device" in _lib.lib().orbx_last_error()
    _check_refusals()


def test_a_problem_without_pairs_returns_its_start(so_path):
    p = scenes.problem(1, 0, fix_scale=True)
    (r, kept), = s3.optimize_sim3([_dev(p)], ISG)
    assert len(kept) == 0 and (r.nin, r.nbad, r.ncorrespondences, tuple(r.iterations)) == (0, 0, 0, (0, 0))
    assert np.array_equal(np.array(list(r.q) + list(r.t) + [r.s]), so.from_rts(p["R12"], p["t12"], p["s12"]).vec())
    assert s3.optimize_sim3([], ISG) == [] and s3.last_sim3_opt_waits() == 0


def build_smoke(tmp_path):
    _lib.build()
    exe = str(tmp_path / "sim3_opt_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wno-reorder", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "sim3_opt_smoke.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_wrapper_fails_loudly_without_a_device(tmp_path):
    """the smoke program compiles against the headers and links; without a device its call returns ORBX_ERR_NO_DEVICE cleanly
    (with one, the program's device run)"""
    import torch
    gpu = torch.cuda.is_available()
    out = subprocess.run([build_smoke(tmp_path)] + ([] if gpu else ["nodevice"]), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ("OK two problems" if gpu else "OK nodevice") in out.stdout


def test_smoke_scene_is_what_the_program_expects():
    """the program's expectations (three pairs cut, the similarity to 1e-4) hold on the restatement"""
    for fixed in (False, True):
        p = scenes.exact(fix_scale=fixed)
        o = so.optimize(p, ISG)
        assert o["res"].nbad == 3 and o["res"].nin == 57 and np.array_equal(~o["kept"], p["bad"])
        assert np.abs(sm.quat_matrix(o["res"].q) - p["R"]).max() < 1e-5 and abs(o["res"].s - p["s"]) < 1e-5


def test_integration_shell_calls_the_declared_entry_points():
    """integration/Optimizer_sim3_hip.cc cannot be compiled here (no OpenCV / g2o): the library calls it makes have the declared
    numbers of arguments, every ORBM_ / ORBX_ constant it names exists, and the documents list it"""
    import test_cpu_integration_shells as shells
    decl, header_text = shells._declarations()
    src = open(os.path.join(ROOT, "integration", "Optimizer_sim3_hip.cc")).read()
    calls = [c for c in shells._calls(src) if c[0] in decl]
    assert ("orbm_optimize_sim3", 6) in calls and decl["orbm_optimize_sim3"] == 6
    assert all(decl[f] == n for f, n in calls), calls
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", shells._strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    body = hpp[hpp.index("inline int OptimizeSim3("):]
    assert ("orbm_optimize_sim3", 6) in [c for c in shells._calls(body) if c[0] in decl]
    assert "HipOptimizeSim3" in shells._strip_comments(src)
    assert "Optimizer_sim3_hip.cc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Optimizer_sim3_hip.cc" in open(os.path.join(ROOT, "integration", "README.md")).read()
