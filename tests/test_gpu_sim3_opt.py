"""OptimizeSim3 on the device (orbm_optimize_sim3, orbm_sim3opt.hip):

* every shape -- n = 0, 1, 9, 10, 11 (the < 10 rule), 63, 64, 65 (a wave's edge), 257, 300 (a 256-thread workgroup's edge), scale
  free and fixed, th2 = 10 -- and the problem at the size limit against the CPU restatement (tests/sim3_opt_oracle.c): (q, t, s)
  within M = 8 times the restatement's own sensitivity D_cpu (tests/golden/sim3_opt_sensitivity.json, measured on the restatement
  alone), the integers equal wherever the restatement's margins are respected (skipped scenes counted, cap 2 %);
* without the restatement: from the device's Sim3, an analytic Gauss-Newton step (tests/sim3_optimum.py) is small and buys nothing;
* the same bytes alone, as problem 0, 31 and 63 of a ragged 64-batch, and on a second call; exactly one host wait;
* NaN and degenerate input: the restatement's outputs and ORBX_OK (bounded arithmetic: every loop of the kernel has a fixed limit).
"""
import json
import subprocess

import numpy as np
import pytest

import sim3_opt_oracle as so
import sim3_opt_scenes as scenes
import sim3_optimum as sm
from orb_slam2_e_amd import sim3 as s3
from test_cpu_sim3_opt import CAP, GOLDEN, M, _check_refusals, _dev, _ints, build_smoke

pytestmark = pytest.mark.gpu

ISG = scenes.INV_SIGMA2
D_CPU = json.load(open(GOLDEN))["D_cpu"]


def _vec(r):
    return np.array(list(r.q) + list(r.t) + [r.s])


def _bytes(r, kept):
    return bytes(r) + kept.tobytes()


@pytest.fixture(scope="module")
def reference():
    """the restatement's result of every scene, computed once"""
    sc = scenes.gpu_scenes()
    return sc, [so.optimize(p, ISG) for p in sc]


@pytest.fixture(scope="module")
def device(reference):
    """every scene as a call of its own"""
    out = []
    for p in reference[0]:
        (r, kept), = s3.optimize_sim3([_dev(p)], ISG)
        out.append((r, kept, s3.last_sim3_opt_waits()))
    return out


def test_scenes_cover_the_shapes(reference):
    sc = reference[0]
    assert sorted({p["n"] for p in sc}) == sorted(scenes.SHAPES + (8192,))
    for n in scenes.SHAPES:
        assert {p["fix_scale"] for p in sc if p["n"] == n} == {0, 1}
    assert all(float(p["th2"]) == 10.0 for p in sc)


def test_sim3_agrees_with_the_restatement_within_eight_times_its_sensitivity(reference, device):
    worst = 0.0
    for p, ref, (r, kept, waits) in zip(*reference, device):
        assert waits == (1 if p["n"] else 0)
        if p["n"] == 0:
            assert np.array_equal(_vec(r), ref["res"].vec())
            continue
        d = float(np.max(np.abs(_vec(r) - ref["res"].vec()) / np.abs(ref["res"].vec())))
        print(p["name"], "relative difference %.3e" % d)
        worst = max(worst, d)
        assert d <= M * D_CPU, (p["name"], d, M * D_CPU)
    print("largest relative difference of (q, t, s) to the restatement: %.3e (8 D_cpu = %.3e)" % (worst, M * D_CPU))


def test_integers_equal_the_restatement_where_its_margins_hold(reference, device):
    """kept, nin, nbad, iterations and trials.  A scene is skipped where the restatement has a cut within M D_cpu th2 of th2 or a
    trial with |rho| below 1e-9 (there the decision is rounding); the skipped scenes are counted and capped."""
    skipped = []
    for p, ref, (r, kept, _) in zip(*reference, device):
        cc = ref["cut_chi"]
        th2 = float(p["th2"])
        if np.sum(np.abs(cc[~np.isnan(cc)] - th2) < M * D_CPU * th2) or ref["trace"].small_rho:
            skipped.append(p["name"])
            continue
        assert _ints(r) == _ints(ref["res"]), p["name"]
        assert np.array_equal(kept, ref["kept"]), p["name"]
    print("skipped:", skipped)
    assert len(skipped) <= CAP * len(reference[0])


def test_device_result_is_the_optimum_of_an_analytic_model(reference, device):
    """Without the restatement's arithmetic: from the device's Sim3, one float64 Gauss-Newton step with analytic Jacobians on the
    pairs the second round optimised is below STEP_TOL and gains less than GAIN_TOL (the bounds of tests/test_gpu_pose_edges.py,
    unscaled; tests/test_cpu_sim3_opt.py says why).  Those pairs are the device's kept ones where its final cut removed none
    (nin = ncorrespondences - nbad); where it removed some, they are the restatement's second-round set, which stands for the
    device's once the first cut is seen to be the same."""
    ran = own = 0
    for p, ref, (r, kept, _) in zip(*reference, device):
        if r.ncorrespondences - r.nbad < 10:
            continue
        if r.nin == r.ncorrespondences - r.nbad:
            active = kept
            own += 1
        else:
            active = ~np.isnan(ref["cut_chi"][1, :, 0])
            assert r.nbad == ref["res"].nbad and not (kept & ~active).any()
        step, gain, cost = sm.gauss_newton_check(p, ISG, active, r.q, r.t, r.s)
        print(p["name"], "step %.2e gain %.2e" % (step, gain))
        assert step <= sm.STEP_TOL and gain <= sm.GAIN_TOL, (p["name"], step, gain)
        assert abs(cost - r.chi2) <= 1e-3 * cost
        ran += 1
    assert ran >= 12 and own >= 6


def test_size_limit():
    big = scenes.problem(2, 8193)
    with pytest.raises(Exception) as e:
        s3.optimize_sim3([_dev(big)], ISG)
    assert e.value.code == -5 and s3.last_sim3_opt_waits() == 0


def test_refusals_with_a_device():
    _check_refusals()


def test_same_bytes_alone_in_a_ragged_batch_and_on_a_second_call(reference, device):
    sc = reference[0]
    pick = [p for p in sc if p["n"] == 65 and not p["fix_scale"]][0]
    alone = [d for p, d in zip(sc, device) if p is pick][0]
    others = [p for p in sc if p["n"] <= 300 and p is not pick]
    batch = [others[k % len(others)] for k in range(64)]
    for slot in (0, 31, 63):
        batch[slot] = pick
    assert len({p["n"] for p in batch}) >= 8
    first = s3.optimize_sim3([_dev(p) for p in batch], ISG)
    assert s3.last_sim3_opt_waits() == 1
    second = s3.optimize_sim3([_dev(p) for p in batch], ISG)
    want = _bytes(alone[0], alone[1])
    for slot in (0, 31, 63):
        assert _bytes(*first[slot]) == want and _bytes(*second[slot]) == want
    for a, b in zip(first, second):
        assert _bytes(*a) == _bytes(*b)
    # every other problem of the batch is what it is alone, too
    by_name = {p["name"]: d for p, d in zip(sc, device)}
    for p, got in zip(batch, first):
        assert _bytes(*got) == _bytes(*by_name[p["name"]][:2]), p["name"]


def _same_as_restatement(p):
    ref = so.optimize(p, ISG)
    (r, kept), = s3.optimize_sim3([_dev(p)], ISG)
    assert s3.last_sim3_opt_waits() == 1
    assert _ints(r) == _ints(ref["res"]) and np.array_equal(kept, ref["kept"]), p["name"]
    return r, ref["res"]


def test_nan_position_returns_the_restatements_outputs():
    p = scenes.nan_position()
    r, ref = _same_as_restatement(p)
    assert r.nin == p["n"] and np.isnan(r.chi2) and np.array_equal(_vec(r), ref.vec())          # the start, bit for bit


def test_all_outliers_and_fewer_than_ten_pairs_return_the_restatements_outputs():
    for p in [scenes.all_outliers()] + [scenes.problem(40 + n, n, outliers=0.5) for n in range(1, 10)]:
        r, ref = _same_as_restatement(p)
        assert r.nin == 0 and np.array_equal(_vec(r), ref.vec())                                 # :1595: the Sim3 as it came in


def test_quirk_scenes_of_the_iteration_allowance():
    for p in (scenes.exact(), scenes.problem(521, 12, noise=0.5, outliers=0.0, off_deg=30.0, off=0.4, th2=1e6)):
        r, ref = _same_as_restatement(p)
        assert float(np.max(np.abs(_vec(r) - ref.vec()) / np.abs(ref.vec()))) <= M * D_CPU


def test_fixed_scale_leaves_the_scale_bit_for_bit(reference, device):
    for p, (r, _, _) in zip(reference[0], device):
        if p["fix_scale"]:
            assert r.s == float(p["s12"])


def test_cxx_wrapper_on_the_device(tmp_path):
    out = subprocess.run([build_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK two problems")
