"""orbm_essential_graph_env, the part that needs no device: orbm_eg_env_plan -- its common outputs against
orbm_eg_plan's, the envelope against one derived in numpy from the pair list, what an ordering costs, the limits by plan alone --, the
scenes of tests/essential_graph_env_scenes.py against the selection rule and their goldens, the ABI surface and the integration shell."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import essential_graph_compare as compare
import essential_graph_env_scenes as ES
import essential_graph_oracle as oracle
import essential_graph_scenes as scenes
import llt_env_reference as E
from orb_slam2_e_amd import _lib, bundle
from orb_slam2_e_amd import essential_graph as EG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSUPPORTED = -5
T = 64
COMMON = ("vertex_class", "row", "vert_edge_start", "vert_edges", "pair_start", "pair_v", "pair_edges")


def numpy_first(g, p):
    """the envelope from the plan's pair list: row tile R starts at the smallest column tile any block that reaches into it has"""
    nact = int((p["vertex_class"] == 0).sum())
    nt = (7 * nact + T - 1) // T
    first = np.arange(nt)
    blocks = [(r, r) for r in range(nact)] + [(int(p["row"][b]), int(p["row"][a])) for a, b in p["pair_v"]]      # (block row, block column)
    for rb, cb in blocks:
        assert rb >= cb
        for R in range(7 * rb // T, (7 * rb + 6) // T + 1):
            first[R] = min(first[R], 7 * cb // T)
    return first.astype(np.int32)


def test_common_outputs_equal_the_dense_plan_and_the_envelope_follows_the_pairs():
    assert bundle.llt_tile() == T
    for name, g in scenes.scenes() + [(n, ES.scene(n)) for n in ES.MID_NAMES] + [("chain(438)", scenes.chain(438))]:
        a, b = EG.plan(g), EG.plan_env(g)
        for k in COMMON:
            assert np.array_equal(a[k], b[k]), (name, k)
        first = numpy_first(g, b)
        assert np.array_equal(b["first"], first), name
        n = 7 * int((b["vertex_class"] == 0).sum())
        want = E.plan(n, first, T)
        assert (b["row_tiles"], b["live_tiles"], b["launches"]) == (len(first), want["live_tiles"], want["launches"]), name


def test_the_new_scenes_have_tiles_off_the_band_among_free_vertices():
    """chain()'s only loop edge ends at the fixed vertex and leaves a pure band; the new scenes do not"""
    band = EG.plan_env(scenes.chain(438))["first"]
    assert (band >= np.arange(len(band)) - 2).all()
    for n in ES.MID_NAMES + [ES.PAST]:
        g = ES.scene(n)
        p = EG.plan_env(g)
        f = p["first"]
        assert (f < np.arange(len(f)) - 3).any(), n
        free = p["vertex_class"][g["e_v0"]] == 0
        far = np.abs(p["row"][g["e_v0"]] - p["row"][g["e_v1"]]) > 20
        assert (free & (p["vertex_class"][g["e_v1"]] == 0) & far & (g["e_kind"] == 0)).sum() >= 3, n     # LoopConnections between neighbours
        assert (free & (p["vertex_class"][g["e_v1"]] == 0) & far & (g["e_kind"] == 1)).sum() >= 2, n     # old loop edges
    p = EG.plan_env(ES.scene(ES.PAST))
    assert (p["vertex_class"] == 0).sum() == 450 and p["row_tiles"] == 50 and (7 * 450) % T != 0
    assert [(ES.scene(n)["fix_scale"], int((EG.plan_env(ES.scene(n))["vertex_class"] == 0).sum())) for n in ES.MID_NAMES] == \
        [(1, 75), (0, 75), (1, 150), (0, 150)]


def test_what_an_ordering_costs_and_the_refusal_past_the_tile_cap():
    g = ES.long_chain(2048)
    p = EG.plan_env(g)
    assert p["row_tiles"] == 224 and p["live_tiles"] < 4 * 224 + 3 * 224                        # id order: a narrow band and three loop rows
    small, _ = ES.shuffled(scenes.chain(438))
    ps = EG.plan_env(small)
    assert ps["live_tiles"] > 0.9 * 48 * 49 // 2 > 7 * EG.plan_env(scenes.chain(438))["live_tiles"]      # shuffled: nearly the whole triangle
    shuffled, _ = ES.shuffled(g)
    with pytest.raises(_lib.OrbxError) as e:
        EG.plan_env(shuffled)
    assert e.value.code == ERR_UNSUPPORTED and "8,192 live tiles" in str(e.value)


def test_limits_by_plan_alone():
    p = EG.plan_env(scenes.chain(4096))
    assert (p["vertex_class"] == 0).sum() == 4096 and p["row_tiles"] == 448 and p["live_tiles"] <= 8192 and p["launches"] <= 4 * 448 - 1
    g = scenes.chain(4097)
    first = np.full(4, -7, np.int32); counts = np.full(6, -7, np.int32)
    cg = EG.c_graph(g)
    rc = _lib.lib().orbm_eg_env_plan(C.byref(cg), None, None, None, None, None, None, None, _lib.ptr(first), _lib.ptr(counts))
    assert rc == ERR_UNSUPPORTED and b"4,096" in _lib.lib().orbx_last_error() and (first == -7).all() and (counts == -7).all()
    base = scenes.chain(40)
    many = dict(base)
    many.update(poses=np.tile(base["poses"][:1], (8193, 1)), fixed=np.zeros(8193, np.uint8), corrected=np.full(8193, -1, np.int32),
                noncorrected=np.full(8193, -1, np.int32))
    for graph, word in ((many, "8,192 keyframes"),
                        (dict(base, e_v0=np.resize(base["e_v0"], 131073), e_v1=np.resize(base["e_v1"], 131073), e_kind=np.resize(base["e_kind"], 131073)), "131,072 edges")):
        with pytest.raises(_lib.OrbxError) as e:
            EG.plan_env(graph)
        assert e.value.code == ERR_UNSUPPORTED and word in str(e.value), word
    ok = dict(many)
    ok.update(poses=many["poses"][:8192], fixed=many["fixed"][:8192], corrected=many["corrected"][:8192], noncorrected=many["noncorrected"][:8192])
    assert EG.plan_env(ok)["row_tiles"] == EG.plan_env(base)["row_tiles"]
    with pytest.raises(_lib.OrbxError) as e:                                                     # the dense entry keeps its own limits
        EG.plan(scenes.chain(439))
    assert "438" in str(e.value)


# ------------------------------------------------------------------------------------------------ sensitivity and goldens
def test_sensitivity_is_the_pinned_one_and_no_scene_decides_at_the_rounding_floor():
    """The 75-vertex scenes are measured again in both forms; of the 150-vertex scenes form 1 alone (the rule and d1): their form 2 --
    34 runs of 20 iterations at n = 1,050 -- takes two minutes and is reproduced by running tests/essential_graph_env_scenes.py, which
    writes the golden.  The next test measures again, with fewer seeds, the one form-2 run that sets D_env."""
    gold = json.load(open(ES.GOLDEN))
    small, (_, _, rows_large) = ES.MID_NAMES[:2], ES.measure(ES.MID_NAMES[2:], form2=False)
    D, each, rows = ES.measure(small)
    rows += rows_large
    print("75 vertices: D %.3e" % D, {k: "%.3e" % v for k, v in each.items()}, [(r["name"], r["iterations"], r["trials"], r["d1"]) for r in rows])
    floor = [r["name"] for r in rows if r["moved"] or r["small_rho"]]
    assert len(floor) <= compare.CAP * len(rows) and floor == []
    assert all(r["lam"] == 0.0 for r in rows)                                                    # lambda keeps its bits under every pattern
    assert gold["scenes"] == [r["name"] for r in rows] == ES.MID_NAMES and gold["ulp_seeds"] == compare.ULP_SEEDS and gold["iter1"] == ES.ITER1
    for r in rows:
        assert gold["d1"][r["name"]] / 2 <= r["d1"] <= gold["d1"][r["name"]] * 2, r
        if r["name"] in small:
            assert gold["d2"][r["name"]] / 2 <= r["d2"] <= gold["d2"][r["name"]] * 2, r
    assert gold["D_env"] == max(max(gold["d1"].values()), max(gold["d2"].values())) and 1e-8 < gold["D_env"] < 1e-3
    assert any(r["trials"] > r["iterations"] for r in rows)                                      # rejected trials are among them


def test_the_run_that_sets_d_env_is_measured_again_with_fewer_seeds():
    """D_env is form 2 of mid150_free under 16 patterns.  Its unperturbed run is pinned ([iterations, trials]) and its sensitivity
    under the FIRST 4 patterns is measured here: within a factor 2 of the pinned figure for those 4, which is at most the full
    figure (a subset's maximum) and of its order -- so a D_env ten times too large would show."""
    gold = json.load(open(ES.GOLDEN))
    pin = gold["d_env_scene"]
    assert pin["scene"] == ES.SETS_D_ENV and pin["seeds"] == ES.FEW_SEEDS and gold["D_env"] == gold["d2"][pin["scene"]]
    d, run = ES.form2_few_seeds()
    print("form 2 of %s under %d patterns: %.3e (pinned %.3e; D_env under 16: %.3e), run %s" % (pin["scene"], pin["seeds"], d, pin["d2_first_seeds"], gold["D_env"], run))
    assert run == pin["form2_run"]
    assert pin["d2_first_seeds"] / 2 <= d <= pin["d2_first_seeds"] * 2
    assert pin["d2_first_seeds"] <= gold["D_env"] <= 10 * pin["d2_first_seeds"]


def test_the_tile_cap_is_checked_behind_the_arguments():
    """the envelope entry's own refusal has the place the size limits have: behind every ORBX_ERR_ARG, before the device"""
    g, _ = ES.shuffled(ES.long_chain(2048))
    cg = EG.c_graph(g)
    nv, npts = len(g["poses"]), len(g["points"])
    poses = np.full((nv, 16), 7, np.float32); points = np.full((npts, 3), 7, np.float32)
    res = EG.EgResult(_lib.ptr(poses), _lib.ptr(points))
    call = _lib.lib().orbm_essential_graph_env
    for opt, code in ((EG.default_options(65), -1), (EG.default_options(20, -1.0), -1), (EG.default_options(20), ERR_UNSUPPORTED),
                      (EG.default_options(0), ERR_UNSUPPORTED)):
        assert call(C.byref(cg), C.byref(opt), C.byref(res), None) == code, (opt.iterations, opt.lambda_init)
    assert b"8,192 live tiles" in _lib.lib().orbx_last_error()
    assert (poses == 7).all() and (points == 7).all()                                            # nothing written


def test_the_450_vertex_golden_belongs_to_its_scene():
    """the digest of the inputs, and the restatement once at the golden's iteration count (about ten seconds)"""
    gold = json.load(open(ES.GOLDEN))["past450"]
    g = ES.scene(ES.PAST)
    assert gold["scene"] == ES.PAST and gold["sha256"] == ES.digest(g) and gold["iterations"] == ES.ITER1[ES.PAST]
    r, z = oracle.run(g, ES.ITER1[ES.PAST], want_system=False), ES.golden_450()
    assert compare.ints(r) == compare.ints(z)
    for k in ("poses", "points", "estimates", "chi2", "trial_log"):
        assert r[k].tobytes() == z[k].tobytes(), k
    assert not (np.abs(z["trial_log"]["rho"]) < compare.RHO_FLOOR).any()
    assert os.path.getsize(ES.GOLDEN_450) < 1 << 20


# ------------------------------------------------------------------------------------------------ text and ABI
def test_entry_points_are_declared_exported_and_bound():
    protos = _lib.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_essential_graph_env"] == protos["orbm_essential_graph"] == (i, [vp] * 4)
    assert protos["orbm_eg_env_plan"] == (i, [vp] * 10) and protos["orbm_eg_plan"] == (i, [vp] * 9)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()]).decode()
    for fn in ("orbm_essential_graph_env", "orbm_eg_env_plan"):
        assert f" T {fn}\n" in out and callable(getattr(_lib.lib(), fn)), fn
    assert _lib.lib().orbx_abi_version() == 136
    for f in (EG.optimize_env, EG.plan_env):
        assert callable(f)
    import orb_slam2_e_amd
    assert orb_slam2_e_amd.optimize_essential_graph_env is EG.optimize_env
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    assert "bool OptimizeEnv(" in hpp and "orbm_essential_graph_env" in hpp


def test_one_body_serves_both_entries():
    src = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_essential_graph.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*\{\};", src, re.M)) == 1
    assert len(re.findall(r"return eg_run\(g, opt, out, stats, (?:true|false)\);", src)) == 2
    assert src.count("system_entry(D, ") == 1 and "const int p0 = D.col_start[cb], p1 = D.col_start[cb + 1];" in src   # k_eg_assemble is as it was


def test_the_new_shell_calls_the_declared_entry_point_and_the_old_one_is_unchanged():
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, header_text = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_essential_graph_env_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert calls.count(("orbm_essential_graph_env", 4)) == 1 and ("orbm_essential_graph", 4) not in calls
    for fn, n in calls:
        assert decl[fn] == n and hasattr(_lib.lib(), fn), fn
    for f, _ in EG.EgGraph._fields_:
        assert f"g.{f} =" in src, f
    for f, _ in EG.EgResult._fields_:
        assert src.count(f"res.{f} = ") == 1, f
    assert "ORBM_EG_OPTIONS_DEFAULT" in src and "bool HipOptimizeEssentialGraphEnv(" in src
    assert "a->mnId < b->mnId" in src and src.index("std::sort(") < src.index("kfIndex[pKF] =")          # sorted before flattening
    call = src.index("orbm_essential_graph_env(")
    before, after = src[:call], src[call:]
    assert not re.search(r"->\w+\s*=[^=]", before) and "SetPose" not in before and "SetWorldPos" not in before and "UpdateNormalAndDepth" not in before
    assert after.index("return false;") < after.index("mMutexMapUpdate") < after.index("SetPose") < after.index("SetWorldPos")
    assert src.count("return false;") == 2 and "8192" in before
    for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert tok in header_text or tok in open(os.path.join(ROOT, "include", "orbslam_hip.h")).read(), tok
    old = open(os.path.join(ROOT, "integration", "Optimizer_essential_graph_hip.cc"), "rb").read()
    assert hashlib.sha256(old).hexdigest() == "24a6359738c066764de725affd7faa70440920c53c2a9a934447c673b399a0fb"
    assert "HipOptimizeEssentialGraphEnv" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
    for doc in ("INTEGRATION.md", os.path.join("integration", "README.md")):
        assert "HipOptimizeEssentialGraphEnv" in open(os.path.join(ROOT, doc)).read(), doc
