"""Optimizer::OptimizeEssentialGraph on the device, the part that needs no device: the ABI surface of orbm_essential_graph /
orbm_eg_plan (declared, exported, bound, struct mirrors = C layout, the documented initialiser), the host planning against lists built
in numpy, every refusal before any device work with the outputs untouched, the limit of 438 vertices in the system, known answers of
the CPU restatement (tests/essential_graph_oracle.c), its sensitivity to the last bit of sin / cos / acos / log / exp pinned in
tests/golden/eg_sensitivity.json (tests/test_gpu_essential_graph.py takes its tolerance from there) with the scenes held to the
selection rule, and the text of the integration shell."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import essential_graph_compare as compare
import essential_graph_optimum as optimum
import essential_graph_oracle as oracle
import essential_graph_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import essential_graph as EG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -5


@pytest.fixture(scope="module")
def so_path():
    return _lib.build()


# ------------------------------------------------------------------------------------------------ 1. the ABI
def test_new_entry_points_are_declared_exported_and_bound(so_path):
    protos = _lib.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_essential_graph"] == (i, [vp] * 4)
    assert protos["orbm_eg_plan"] == (i, [vp] * 9)
    assert protos["orbm_debug_last_eg_waits"] == (i, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for fn in ("orbm_essential_graph", "orbm_eg_plan", "orbm_debug_last_eg_waits"):
        assert f" T {fn}\n" in out, fn
    assert _lib.lib().orbx_abi_version() == 136


def test_struct_mirrors_and_the_initialiser_have_the_c_values(tmp_path):
    exe = str(tmp_path / "abi_layout_eg")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_eg.c"), "-o", exe])
    sizes, fields, opts = {}, {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        elif w[0] == "field":
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
        else:
            opts[w[1]] = [float(x) for x in w[2:]]
    for m, name in ((EG.EgGraph, "orbm_eg_graph"), (EG.EgOptions, "orbm_eg_options"), (EG.EgResult, "orbm_eg_result"), (EG.EgStats, "orbm_eg_stats"),
                    (oracle.Graph, "orbm_eg_graph"), (oracle.Options, "orbm_eg_options")):
        assert C.sizeof(m) == sizes[name], name
        assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name], name
    assert oracle.TRIAL_DTYPE.itemsize == sizes["orbm_ba_trial"]
    o = EG.default_options()
    assert [o.iterations, o.reserved, o.lambda_init] == opts["default"] == [20, 0, 1e-16]
    assert EG.ITERATIONS == 20 and "#define ORBM_EG_ITERATIONS 20" in open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()


# ------------------------------------------------------------------------------------------------ 2. the host planning
def _numpy_plan(g):
    nv = len(g["poses"])
    e0, e1 = g["e_v0"], g["e_v1"]
    cls = np.full(nv, 2, np.int32)
    cls[np.unique(np.concatenate([e0, e1]))] = 0
    cls[g["fixed"] != 0] = 1
    row = np.full(nv, -1, np.int32); row[cls == 0] = np.arange((cls == 0).sum())
    vert_edges = []
    for v in range(nv):
        codes = sorted([2 * int(e) for e in np.nonzero(e0 == v)[0]] + [2 * int(e) + 1 for e in np.nonzero(e1 == v)[0]]) if cls[v] == 0 else []
        vert_edges.append(codes)
    pairs = {}
    for e, (a, b) in enumerate(zip(e0, e1)):
        if row[a] < 0 or row[b] < 0:
            continue
        key = (int(a), int(b)) if row[a] < row[b] else (int(b), int(a))
        pairs.setdefault(key, []).append(2 * e + (1 if row[a] > row[b] else 0))
    return cls, row, vert_edges, pairs


@pytest.mark.parametrize("name", ["two_v0fixed_fix", "two_v1fixed_free", "ring9_fix", "ring10_free", "tree40_fix", "tree70_free"])
def test_plan_gives_the_lists_built_in_numpy(name):
    g = scenes.scene(name)
    p = EG.plan(g)
    cls, row, vert_edges, pairs = _numpy_plan(g)
    nv = len(g["poses"])
    assert np.array_equal(p["vertex_class"], cls) and np.array_equal(p["row"], row)
    for v in range(nv):
        assert p["vert_edges"][p["vert_edge_start"][v]:p["vert_edge_start"][v + 1]].tolist() == vert_edges[v], v
    assert p["vert_edge_start"][nv] == len(p["vert_edges"])
    keys = sorted(pairs, key=lambda k: (row[k[0]], row[k[1]]))
    assert p["pair_v"].tolist() == [list(k) for k in keys]                       # ascending by (smaller row, larger row)
    for k, key in enumerate(keys):
        assert p["pair_edges"][p["pair_start"][k]:p["pair_start"][k + 1]].tolist() == pairs[key], key
    assert p["pair_start"][len(keys)] == len(p["pair_edges"])
    if name.startswith("tree40"):
        assert (cls == 2).sum() == 1 and cls[5] == 2 and (cls == 0).sum() == 39                 # the keyframe without an edge
        assert cls[17] == 1 and 0 < 17 < nv - 1                                                   # the fixed vertex inside the list
        double = [v for v in pairs.values() if len(v) == 2]
        assert len(double) == 1 and sorted(c & 1 for c in double[0]) == [0, 1]                   # one pair, both orientations
        assert set(g["e_kind"].tolist()) == {0, 1} and (g["corrected"] >= 0).sum() == 3 and (g["noncorrected"] >= 0).sum() == 3
    if name.startswith("ring10"):
        assert 7 * (cls == 0).sum() == 70                                                         # the last block straddles row 64


# ------------------------------------------------------------------------------------------------ 3. refusals and limits
def _call(g, sizes=None, null=(), iterations=20, lambda_init=1e-16, null_out=()):
    """orbm_essential_graph with sentinel-filled outputs; returns (rc, outputs untouched)"""
    L = _lib.lib()
    cg = EG.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    for k in null:
        setattr(cg, k, None)
    nv, npts = len(g["poses"]), len(g["points"])
    poses = np.full((nv + 1100, 16), 7.5, np.float32); points = np.full((npts + 1, 3), 7.5, np.float32)
    res = EG.EgResult(None if "poses" in null_out else EG.ptr(poses), None if "points" in null_out else EG.ptr(points))
    opt = EG.default_options(iterations, lambda_init)
    rc = L.orbm_essential_graph(C.byref(cg), C.byref(opt), C.byref(res), None)
    return rc, bool((poses == 7.5).all() and (points == 7.5).all())


def test_every_refusal_comes_before_any_device_work_and_writes_nothing():
    g = scenes.scene("tree40_free")
    for sizes in ({"nvert": 1025}, {"nedges": 32769}, {"npoints": 1048577}):
        assert _call(g, sizes) == (ERR_UNSUPPORTED, True), sizes
    for sizes in ({"nvert": -1}, {"ncorr": -1}, {"nnc": -1}, {"nedges": -1}, {"npoints": -1}):
        assert _call(g, sizes) == (ERR_ARG, True), sizes
    for null in ("poses", "corrected", "corrected_sim3", "noncorrected", "noncorrected_sim3", "fixed", "e_v0", "e_v1", "e_kind", "points", "p_ref"):
        assert _call(g, null=(null,)) == (ERR_ARG, True), null
    for null_out in ("poses", "points"):
        assert _call(g, null_out=(null_out,)) == (ERR_ARG, True), null_out

    def edited(key, index, value):
        h = dict(g)
        a = g[key].copy(); a.reshape(-1)[index] = value
        h[key] = a
        return h
    nv = len(g["poses"])
    for key, bad in (("e_v0", -1), ("e_v0", nv), ("e_v1", -1), ("e_v1", nv), ("p_ref", -1), ("p_ref", nv), ("corrected", 3), ("corrected", -2),
                     ("noncorrected", 3), ("e_kind", 2)):
        assert _call(edited(key, 4, bad)) == (ERR_ARG, True), (key, bad)
    assert _call(edited("e_v1", 4, g["e_v0"][4])) == (ERR_ARG, True)                             # e_v0 == e_v1
    assert b"itself" in _lib.lib().orbx_last_error()
    fixed_pair = dict(g); f = g["fixed"].copy(); f[g["e_v0"][4]] = 1; f[g["e_v1"][4]] = 1; fixed_pair["fixed"] = f
    assert _call(fixed_pair) == (ERR_ARG, True)                                                   # an edge between two fixed vertices
    assert b"two fixed" in _lib.lib().orbx_last_error()
    for key, index in (("poses", 7), ("corrected_sim3", 9), ("noncorrected_sim3", 2), ("points", 5)):
        for bad in (float("nan"), float("inf")):
            assert _call(edited(key, index, bad)) == (ERR_ARG, True), (key, bad)
    for it in (-1, 65):
        assert _call(g, iterations=it) == (ERR_ARG, True)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(g, lambda_init=lam) == (ERR_ARG, True)
    # the planning entry refuses the same graphs
    cg = EG.c_graph(g); cg.nvert = 1025
    assert _lib.lib().orbm_eg_plan(C.byref(cg), None, None, None, None, None, None, None, None) == ERR_UNSUPPORTED


def test_438_vertices_in_the_system_are_accepted_and_439_refused():
    """7 * 438 = 3,066 <= 3,072, the solver's limit (tests/test_cpu_llt.py pins it); 7 * 439 = 3,073"""
    L = _lib.lib()
    at, over = scenes.chain(438, edges_per_vertex=2), scenes.chain(439, edges_per_vertex=2)
    counts = np.zeros(3, np.int32)
    cg = EG.c_graph(at)
    assert L.orbm_eg_plan(C.byref(cg), None, None, None, None, None, None, None, EG.ptr(counts)) == OK
    assert (EG.plan(at)["vertex_class"] == 0).sum() == 438
    cg = EG.c_graph(over)
    assert L.orbm_eg_plan(C.byref(cg), None, None, None, None, None, None, None, None) == ERR_UNSUPPORTED
    assert _call(over) == (ERR_UNSUPPORTED, True) and b"438" in L.orbx_last_error()
    # a 439th free keyframe WITHOUT an edge is not a vertex of the system: accepted (here: up to the device check)
    extra = dict(at)
    extra.update(poses=np.concatenate([at["poses"], at["poses"][:1]]), fixed=np.append(at["fixed"], 0).astype(np.uint8),
                 corrected=np.append(at["corrected"], -1).astype(np.int32), noncorrected=np.append(at["noncorrected"], -1).astype(np.int32))
    p = EG.plan(extra)
    assert p["vertex_class"][-1] == 2 and p["row"][-1] == -1 and (p["vertex_class"] == 0).sum() == 438
    assert _call(extra, iterations=0)[0] in (OK, ERR_NO_DEVICE)


# ------------------------------------------------------------------------------------------------ 4. known answers of the restatement
def test_log_of_exp_returns_the_argument_on_both_sides_of_each_branch():
    """Sim3::log(Sim3(u)) = u.  The bounds are the formulas' own errors:
      theta above the branch (d <= 1 - 1e-5, theta >= 4.47e-3): 1 - cos(theta) loses eps / theta^2; acos(d) loses eps / sin(theta)
        and deltaR, a difference of entries of size 1, another eps / sin(theta) of its 2 sin(theta); the solve with W carries them to
        upsilon in proportion to |u|; with |sigma| >= 1e-5, C = (s - 1) / sigma loses eps / |sigma| more
        -> 64 eps (1 / theta^2 + 1 / sin^2(theta) + [1 / |sigma|]) (1 + |u|)
      theta below it, |sigma| < 1e-5: omega = deltaR / 2 is the first-order form (relative error theta^2 / 6) and A = 1/2, B = 1/6
        are the limits -> theta^2 (1 + |u|)
      theta below it, |sigma| >= 1e-5: the reference's B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (types/sim3.h:199, and :116 in the
        constructor) lacks the - 1 of the closed form and is of order 1 / sigma^3: W is dominated by B Omega^2 and the round trip does
        NOT come back.  Kept as it is; asserted here so that a "correction" does not slip in."""
    eps = 2.0 ** -53
    rng = np.random.default_rng(0)

    def trip(theta, sigma):
        w = rng.standard_normal(3); w *= theta / np.linalg.norm(w)
        u = np.concatenate([w, rng.standard_normal(3), [sigma]])
        return float(np.abs(oracle.sim3_log(oracle.sim3_exp(u)) - u).max()), float(np.abs(u).max())
    for sigma in (0.0, 5e-6, -9e-6, 2e-5, 0.1, -0.3):
        for theta in (4.6e-3, 0.05, 0.3, 2.5):
            err, mag = trip(theta, sigma)
            loss = 1 / theta ** 2 + 1 / np.sin(theta) ** 2 + (1 / abs(sigma) if abs(sigma) >= 1e-5 else 0.0)
            assert err <= 64 * eps * loss * (1 + mag), (theta, sigma, err)
    for sigma in (0.0, 5e-6, -9e-6):
        for theta in (1e-7, 1e-4, 1e-3, 4.4e-3):
            err, mag = trip(theta, sigma)
            assert err <= theta ** 2 * (1 + mag) + 64 * eps, (theta, sigma, err)
    for theta, sigma in ((1e-3, 3e-5), (1e-3, 0.1), (4e-3, -0.01)):
        err, _ = trip(theta, sigma)
        assert err > 1e-4, (theta, sigma, err)


def _model_jacobian(g, M, V, e, side, h=1e-6):
    """float64 central differences of the independent model (tests/essential_graph_optimum.py) for one side of edge e: [7][7]"""
    i, j = g["e_v0"][e], g["e_v1"][e]
    J = np.zeros((7, 7))
    for d in range(7):
        cols = []
        for sgn in (1.0, -1.0):
            u = np.zeros(7); u[d] = sgn * h
            P = optimum.expm(optimum.generator(u))[0] @ V[j if side else i]
            E = M[e] @ (V[i] if side else P) @ np.linalg.inv(P if side else V[j])
            cols.append(optimum.coordinates(optimum.logm(E[None]))[0])
        J[:, d] = (cols[0] - cols[1]) / (2 * h)
    return J


def test_jacobian_columns_are_the_central_differences_of_an_independent_model():
    """g2o's numeric Jacobian steps by 1e-9: its entries carry the rounding of the error (2^-53 times intermediate values of up to ~10)
    divided by 2e-9, about 1e-6; the model steps by 1e-6 (truncation 1e-12) and normalises the quaternions that the reference takes
    unnormalised from a float pose (1e-7 relative).  Bound: 1e-5 absolute on entries of size 1 .. 10, ten times that noise."""
    g = scenes.scene("tree40_free")
    r = oracle.run(g, 1)
    V, M = optimum.start(g)
    assert np.abs(optimum.matrices(r["meas"]) - M).max() <= 1e-6                      # the measurements Sji of both kinds
    worst = 0.0
    for e in (0, 1, 2, 7, 40, 90, len(g["e_v0"]) - 1):
        for side in (0, 1):
            v = (g["e_v1"] if side else g["e_v0"])[e]
            if g["fixed"][v]:
                assert not r["J0"][e, side].any()                                      # a fixed side is skipped
                continue
            worst = max(worst, float(np.abs(r["J0"][e, side] - _model_jacobian(g, M, V, e, side)).max()))
    print("largest Jacobian difference to the model: %.3e" % worst)
    assert worst <= 1e-5


def test_fixed_scale_makes_column_6_and_b6_exactly_zero():
    for name in ("ring9_fix", "tree40_fix"):
        g = scenes.scene(name)
        r = oracle.run(g, 1)
        nact = int((EG.plan(g)["vertex_class"] == 0).sum())
        assert not r["J0"][:, :, :, 6].any() and r["J0"][:, :, :, :6].any()
        assert not r["b0"][:7 * nact].reshape(nact, 7)[:, 6].any() and r["b0"][:7 * nact].any()
    g = scenes.scene("ring9_free")
    r = oracle.run(g, 1)
    assert r["J0"][:, :, :, 6].any()


def test_the_scenes_plant_both_sides_of_the_two_branches_of_the_logarithm():
    """the errors at the start, from the independent model: sigma on both sides of 1e-5, theta on both sides of 4.47e-3"""
    seen = set()
    for name, g in scenes.scenes():
        V, M = optimum.start(g)
        e = optimum.errors(g, M, V)
        theta, sigma = np.linalg.norm(e[:, :3], axis=1), np.abs(e[:, 6])
        seen |= {(bool(t), bool(s)) for t, s in zip(np.cos(theta) > 1 - 1e-5, sigma < 1e-5)}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ------------------------------------------------------------------------------------------------ 5. sensitivity and scene selection
def test_sensitivity_is_the_pinned_one_and_no_scene_decides_at_the_rounding_floor():
    """Form 1 of every scene: no trial with |rho| < 1e-9 and the same integers under all 16 patterns.  12 scenes; 2 % of them is
    none, and none is left out: every scene is compared in its integers on the device."""
    D, rows = compare.measure_sensitivity()
    floor = [r["name"] for r in rows if r["moved"] or r["small_rho"]]
    print("D_cpu %.3e" % D, "scenes:", len(rows), "at the floor:", floor, {k: "%.3e" % v for k, v in compare.D_EACH.items()})
    gold = json.load(open(compare.GOLDEN))
    assert gold["scenes"] == [r["name"] for r in rows] == scenes.NAMES and gold["ulp_seeds"] == compare.ULP_SEEDS
    assert gold["iter1"] == scenes.ITER1
    assert len(floor) <= compare.CAP * len(rows), floor
    assert floor == []
    assert gold["D_cpu"] / 2 <= D <= gold["D_cpu"] * 2, (D, gold["D_cpu"])
    # the numeric Jacobians divide the error's last bits by 2e-9: the sensitivity is of order 1e-16 / 1e-9 times the conditioning
    assert 1e-8 < gold["D_cpu"] < 1e-4
    assert gold["D_cpu"] == max(max(gold["d1"].values()), max(gold["d2"].values()))
    assert set(gold["D_each"]) == set(compare.D_EACH) == {"chi2", "lambda", "tempChi", "currentChi"}
    for k, v in compare.D_EACH.items():
        assert gold["D_each"][k] / 2 <= v <= gold["D_each"][k] * 2 or gold["D_each"][k] == v == 0.0, (k, v, gold["D_each"][k])
        assert gold["D_each"][k] < 1e-6, k
    # the forms: form 1 of the multi-edge scenes runs 3 .. 6 iterations off the floor; one edge is solved by the first step
    for r in rows:
        n = r["base1"]["iterations"]
        assert (n == 1) if r["name"].startswith("two_") else (3 <= n <= 6), (r["name"], n)
    assert any(2 in r["base1"]["results"] for r in rows) and any(not r["base1"]["trial_log"]["accepted"].all() for r in rows)


# ------------------------------------------------------------------------------------------------ 6. the unit and the shell
def test_the_lease_site_has_its_stale_workspace_case():
    """orbm_essential_graph.hip leases ONE pooled workspace, declared as orbm_ba.hip declares its own; its stale-arena case is
    tests/test_gpu_essential_graph_workspace.py, under every fill of the table."""
    src = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_essential_graph.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*(?:\{\})?;", src, re.M)) == 1 and "WorkspaceLease" not in src
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*\{\};", src, re.M)) == 1
    case = open(os.path.join(ROOT, "tests", "test_gpu_essential_graph_workspace.py")).read()
    assert "W.FILLS" in case and "fill_workspaces" in case and "EG.optimize" in case
    mk = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "Makefile")).read()
    assert "orbm_essential_graph.hip" in mk and "-ffp-contract=off" in mk


def test_the_sim3_arithmetic_has_one_definition():
    csrc = os.path.join(ROOT, "orb_slam2_e_amd", "csrc")
    hdr = open(os.path.join(csrc, "orbm_sim3_math.h")).read()
    for fn in ("sim3_exp", "sim3_mul", "sim3_inverse", "struct Sim3"):
        assert fn in hdr
        for unit in ("orbm_sim3opt.hip", "orbm_essential_graph.hip"):
            src = open(os.path.join(csrc, unit)).read()
            assert '#include "orbm_sim3_math.h"' in src
            assert not re.search(r"void\s+" + fn + r"\s*\(", src) and "struct Sim3 {" not in src, (unit, fn)


def test_integration_shell_calls_the_declared_entry_point_and_writes_nothing_before_it():
    """integration/Optimizer_essential_graph_hip.cc cannot be compiled here (no OpenCV): its C-ABI call is declared with that many
    arguments and exported, it sets every member of the graph and of the result, takes the documented initialiser, returns false
    before any write, and holds mMutexMapUpdate around the write-back."""
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, header_text = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_essential_graph_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert calls.count(("orbm_essential_graph", 4)) == 1
    for fn, n in calls:
        assert decl[fn] == n and hasattr(_lib.lib(), fn), fn
    for f, _ in EG.EgGraph._fields_:
        assert f"g.{f} =" in src, f
    for f, _ in EG.EgResult._fields_:
        assert src.count(f"res.{f} = ") == 1, f
    assert "ORBM_EG_OPTIONS_DEFAULT" in src and "bool HipOptimizeEssentialGraph(" in src
    assert "minFeat" in src and "sInsertedEdges" in src and "GetCovisiblesByWeight(minFeat)" in src and "mnCorrectedReference" in src
    call = src.index("orbm_essential_graph(")
    before, after = src[:call], src[call:]
    assert not re.search(r"->\w+\s*=[^=]", before) and "SetPose" not in before and "SetWorldPos" not in before and "UpdateNormalAndDepth" not in before
    assert after.index("return false;") < after.index("mMutexMapUpdate") < after.index("SetPose") < after.index("SetWorldPos")
    assert "UpdateNormalAndDepth" in after and src.count("return false;") == 2
    for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert tok in header_text or tok in open(os.path.join(ROOT, "include", "orbslam_hip.h")).read(), tok
    # it is a file of its own: the patch's hunks and the BA shell stay as they are
    assert "HipOptimizeEssentialGraph" not in open(os.path.join(ROOT, "integration", "Optimizer_ba_hip.cc")).read()
    assert "HipOptimizeEssentialGraph" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
    assert "HipOptimizeEssentialGraph" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
