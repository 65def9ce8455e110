"""orbm_essential_graph_env on the MI355X: Optimizer::OptimizeEssentialGraph on the tile-envelope solver.
  Where the dense entry accepts the graph it is the yardstick, and an exact one: every output EQUAL (np.array_equal; the sign of a
    zero inside the solve is the one thing skipping a zero tile may change) on the 12 scenes of essential_graph_scenes.py in both
    forms and on chain(438).
  Past the dense entry's 438 vertices: the scenes of essential_graph_env_scenes.py (loops among free vertices, off-band tiles) against
    the CPU restatement -- every integer equal, continuous outputs within M = 8 times the restatement's own sensitivity, measured on
    the restatement alone (tests/golden/eg_sensitivity.json, eg_env_sensitivity.json); the 450-vertex scene against its golden; a
    shuffled listing (wide envelope) against the restatement on the shuffled graph.  The issue's bound is M max(D_cpu, D_env), and
    D_env = 7.5e-4 comes from ONE run, the 20 iterations of the free-scale 150-vertex scene; held to it, every other comparison
    would pass with an error a hundred times what it shows.  So each comparison is held to the sensitivity of its OWN kind of run,
    never above the issue's bound: form 1, the shuffled listing and the golden to M max(D_cpu, largest d1 of the scenes), form 2
    of a scene to M max(D_cpu, that scene's d2).
  Without a restatement: 2,048 and 4,096 vertices, and a consistent ring of 600 vertices against its planted configuration."""
import json
import os
import subprocess

import numpy as np
import pytest

import essential_graph_compare as compare
import essential_graph_env_scenes as ES
import essential_graph_optimum as optimum
import essential_graph_oracle as oracle
import essential_graph_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import essential_graph as EG
from test_gpu_essential_graph import _conversion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLD, _GOLD_ENV = json.load(open(compare.GOLDEN)), json.load(open(ES.GOLDEN))
M = compare.M
D = max(_GOLD["D_cpu"], _GOLD_ENV["D_env"])                       # the issue's bound is M D: nothing below is held to more
D1 = max(_GOLD["D_cpu"], max(_GOLD_ENV["d1"].values()))           # form 1 of any scene, the shuffled listing, the golden
assert D1 <= D


def d_form2(name):
    """form 2 of one scene: its own 20-iteration sensitivity"""
    return max(_GOLD["D_cpu"], _GOLD_ENV["d2"][name])


ARRAYS = ("poses", "points", "estimates", "chi2")
LOG_FIELDS = ("tempChi", "currentChi", "rho", "lam", "scale", "round", "qmax", "accepted", "ok2")


def assert_equal_outputs(a, b, what):
    """every output of two results equal as numbers, NaN nowhere"""
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert compare.ints(a) == compare.ints(b) and a["ntrials"] == b["ntrials"] and a["trial_overflow"] == b["trial_overflow"], what
    for f in LOG_FIELDS:
        assert np.array_equal(a["trial_log"][f], b["trial_log"][f]), (what, f)


def assert_same_bytes(a, b, what):
    for k in ARRAYS + ("trial_log",):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ------------------------------------------------------------------------------------------------ the dense entry as yardstick
def test_every_output_equals_the_dense_entry_on_its_scenes():
    for n, g in scenes.scenes():
        for it in (scenes.ITER1[n], scenes.ITER2):
            dense, env = EG.optimize(g, it, want_stats=True), EG.optimize_env(g, it, want_stats=True)
            assert_equal_outputs(env, dense, (n, it))
            assert env["waits"] == env["trials"] + 1 == dense["waits"], (n, it)
    g = scenes.scene("tree70_free")
    a, b = EG.optimize_env(g, scenes.ITER2, want_stats=True), EG.optimize_env(g, scenes.ITER2, want_stats=True)
    assert_same_bytes(a, b, "tree70_free twice")
    none = EG.optimize_env(g, 0, want_stats=True)                                                 # iterations = 0: no solve
    assert none["waits"] == 1 and none["trials"] == 0 and np.array_equal(none["poses"], EG.optimize(g, 0)["poses"])


def test_every_output_equals_the_dense_entry_at_its_limit():
    g = scenes.chain(438)
    p = EG.plan_env(g)
    assert p["row_tiles"] == 48 and p["live_tiles"] < 48 * 49 // 2 // 4                           # a band: a fraction of the triangle
    dense = EG.optimize(g, 2, want_stats=True)
    assert _lib.lib().orbm_debug_last_llt_launches() == 191
    env = EG.optimize_env(g, 2, want_stats=True)
    assert _lib.lib().orbm_debug_last_llt_launches() == p["launches"] <= 191
    assert_equal_outputs(env, dense, "chain(438)")
    assert env["waits"] == env["trials"] + 1
    assert_same_bytes(EG.optimize_env(g, 2, want_stats=True), env, "chain(438) twice")


def test_a_graph_past_the_dense_limit_is_refused_there_and_accepted_here():
    g = scenes.chain(439)
    with pytest.raises(_lib.OrbxError) as e:
        EG.optimize(g, 1)
    assert e.value.code == -5
    r = EG.optimize_env(g, 1, want_stats=True)
    assert r["iterations"] == 1 and r["trial_log"]["ok2"].all() and r["waits"] == r["trials"] + 1


# ------------------------------------------------------------------------------------------------ past the old limit, the restatement
def _held(d, r, what, form, worst, bound):
    assert bound <= D
    if form == 1:
        assert compare.ints(d) == compare.ints(r), what
        assert d["ntrials"] == r["ntrials"] == d["trials"] and not d["trial_overflow"] and d["trial_log"]["ok2"].all(), what
    for k, v in (compare.diffs(d, r) if form == 1 else compare.diffs_final(d, r)).items():
        worst[k] = max(worst.get(k, (0.0, what)), (v, what))
        assert v <= M * bound, (what, form, k, v, M * bound)


def test_mid_size_scenes_agree_with_the_restatement():
    assert _GOLD_ENV["scenes"] == ES.MID_NAMES and _GOLD_ENV["iter1"] == ES.ITER1
    for form in (1, 2):
        worst = {}
        for n in ES.MID_NAMES:
            g, it = ES.scene(n), ES.ITER1[n] if form == 1 else ES.ITER2
            assert (EG.plan_env(g)["first"][2:] < np.arange(2, EG.plan_env(g)["row_tiles"]) - 1).any()      # tiles off the band
            d, r = EG.optimize_env(g, it, want_stats=True), oracle.run(g, it, want_system=False)
            assert d["waits"] == d["trials"] + 1
            _held(d, r, n, form, worst, D1 if form == 1 else d_form2(n))
        print("form %d, largest relative differences to the restatement:" % form, {k: "%.3e (%s)" % v for k, v in worst.items()},
              "bounds:", "%.3e" % (M * D1) if form == 1 else {n: "%.3e" % (M * d_form2(n)) for n in ES.MID_NAMES})


def test_a_shuffled_listing_agrees_with_the_restatement_on_the_shuffled_graph():
    n = "mid150_fix"
    g, _ = ES.shuffled(ES.scene(n))
    assert EG.plan_env(g)["live_tiles"] > 2 * EG.plan_env(ES.scene(n))["live_tiles"]              # a wide envelope
    for form in (1, 2):
        worst = {}
        it = ES.ITER1[n] if form == 1 else ES.ITER2
        bound = D1 if form == 1 else d_form2(n)
        _held(EG.optimize_env(g, it, want_stats=True), oracle.run(g, it, want_system=False), n + " shuffled", form, worst, bound)
        print("shuffled, form %d:" % form, {k: "%.3e" % v[0] for k, v in worst.items()}, "bound %.3e" % (M * bound))


def test_the_450_vertex_scene_agrees_with_its_golden():
    g = ES.scene(ES.PAST)
    assert ES.digest(g) == _GOLD_ENV["past450"]["sha256"] and _GOLD_ENV["past450"]["iterations"] == ES.ITER1[ES.PAST]
    p = EG.plan_env(g)
    assert (p["vertex_class"] == 0).sum() == 450 and p["row_tiles"] == 50 and 7 * 450 % 64 != 0
    d = EG.optimize_env(g, ES.ITER1[ES.PAST], want_stats=True)
    assert _lib.lib().orbm_debug_last_llt_launches() == p["launches"]
    worst = {}
    _held(d, ES.golden_450(), ES.PAST, 1, worst, D1)
    print("450 vertices, largest relative differences to the golden:", {k: "%.3e" % v[0] for k, v in worst.items()}, "bound %.3e" % (M * D1))


# ------------------------------------------------------------------------------------------------ without a restatement
def test_2048_vertices_twice():
    g = ES.long_chain(2048, fix_scale=True, isolated=True)
    p = EG.plan_env(g)
    cls = p["vertex_class"]
    assert (cls == 0).sum() == 2048 and (cls == 1).sum() == 1 and (cls == 2).sum() == 1
    a = EG.optimize_env(g, 2, want_stats=True)
    assert _lib.lib().orbm_debug_last_llt_launches() == p["launches"] <= 4 * p["row_tiles"] - 1
    b = EG.optimize_env(g, 2, want_stats=True)
    assert_same_bytes(a, b, "2,048 vertices twice")
    assert a["iterations"] == 2 and a["waits"] == a["trials"] + 1 and a["trial_log"]["ok2"].all() and a["trial_log"]["accepted"].any()
    start = np.stack([g["corrected_sim3"][g["corrected"][v]] if g["corrected"][v] >= 0 else _conversion(g["poses"][v])[1] for v in range(len(cls))])
    assert a["estimates"][:, 7].tobytes() == start[:, 7].tobytes()                                # the scale is fixed: every scale has its input's bits
    still = np.nonzero(cls != 0)[0]
    assert a["estimates"][still].tobytes() == start[still].tobytes()                              # the fixed and the edgeless vertex
    for v in still:
        assert a["poses"][v].tobytes() == _conversion(g["poses"][v])[0].tobytes(), v
    moved = np.nonzero(cls == 0)[0]
    assert (a["estimates"][moved, :7] != start[moved, :7]).any(axis=1).all()
    V, Mm = optimum.start(g)
    c0, c1 = optimum.cost(g, Mm, V), optimum.cost(g, Mm, optimum.matrices(a["estimates"]))
    print("2,048 vertices: model cost %.6e -> %.6e, trials %d, %d live tiles, %d launches per solve" % (c0, c1, a["trials"], p["live_tiles"], p["launches"]))
    assert c1 < c0


def test_4096_vertices_once():
    g = ES.long_chain(4096)
    p = EG.plan_env(g)
    assert (p["vertex_class"] == 0).sum() == 4096 and p["row_tiles"] == 448
    a = EG.optimize_env(g, 1, want_stats=True)
    assert _lib.lib().orbm_debug_last_llt_launches() == p["launches"] <= 4 * 448 - 1
    assert a["iterations"] == 1 and a["waits"] == a["trials"] + 1 and a["trial_log"]["ok2"].all() and np.isfinite(a["estimates"]).all()
    print("4,096 vertices: trials %d, %d live tiles, %d launches per solve" % (a["trials"], p["live_tiles"], p["launches"]))


def test_a_consistent_ring_of_600_vertices_returns_to_its_planted_configuration():
    """essential_graph_scenes.planted_ring(600): every measurement is consistent with one planted configuration, the start drifts away
    from it.  n = 4,193, past anything a restatement reaches here; the bound is the one tests/test_gpu_essential_graph.py holds the
    10-vertex ring to, scaled as there: 10 times what the restatement reaches on that ring (1.1e-7), 20 iterations."""
    from test_gpu_essential_graph import RESTATEMENT_RING_ERROR
    g, planted = scenes.planted_ring(600)
    assert (EG.plan_env(g)["vertex_class"] == 0).sum() == 599
    start = np.abs(g["poses"].reshape(-1, 4, 4) - optimum.matrices(planted)).max()
    d = EG.optimize_env(g, 20, want_stats=True)
    err = np.abs(optimum.matrices(d["estimates"]) - optimum.matrices(planted)).max()
    print("planted ring of 600: start %.3e device %.3e bound %.3e iterations %d trials %d results %s"
          % (start, err, 10 * RESTATEMENT_RING_ERROR, d["iterations"], d["trials"], d["results"]))
    assert start > 0.05 and d["waits"] == d["trials"] + 1
    assert err <= 10 * RESTATEMENT_RING_ERROR


# ------------------------------------------------------------------------------------------------ the C++ class
def test_through_the_cxx_class(tmp_path):
    libdir = os.path.dirname(_lib.SO_PATH)
    exe = str(tmp_path / "essential_graph_env_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "essential_graph_env_smoke.cpp"), "-o", exe, "-L", libdir, "-lorbslam_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    name = "mid75_free"
    g = ES.scene(name)
    sp, op = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(sp, "wb") as f:
        f.write(np.array([len(g["poses"]), len(g["corrected_sim3"]), len(g["noncorrected_sim3"]), len(g["e_v0"]), len(g["points"]), g["fix_scale"]],
                         np.int32).tobytes())
        for k in ("poses", "corrected", "corrected_sim3", "noncorrected", "noncorrected_sim3", "fixed", "e_v0", "e_v1", "e_kind", "points", "p_ref"):
            f.write(g[k].tobytes())
    out = subprocess.run([exe, sp, op, str(ES.ITER2)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    d = EG.optimize_env(g, ES.ITER2)
    assert open(op, "rb").read() == d["poses"].tobytes() + d["points"].tobytes()
