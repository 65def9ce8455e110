"""Optimizer::LocalBundleAdjustment / BundleAdjustment on the device, the part that needs no device: the ABI surface of
orbm_bundle_adjustment / orbm_ba_plan (declared, exported, bound, struct mirrors = C layout, the two documented initialisers), the
host planning against lists built in numpy, every refusal before any device work with the outputs untouched, known answers of the
CPU restatement (tests/ba_oracle.c), and its sensitivity to the last bit of sin / cos / pow, pinned in
tests/golden/ba_sensitivity.json (tests/test_gpu_ba.py takes its tolerance from there)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import ba_optimum
import ba_oracle
import ba_scenes
from orb_slam2_e_amd import _lib, bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope="module")
def so_path():
    return _lib.build()


@pytest.fixture(scope="module")
def scenes():
    return ba_scenes.scenes()


@pytest.fixture(scope="module")
def reference(scenes):
    """name -> the restatement's result, computed once"""
    return {name: ba_oracle.run(g, opt) for name, g, opt in scenes}


# ------------------------------------------------------------------------------------------------ 1. the ABI
def test_new_entry_points_are_declared_exported_and_bound(so_path):
    protos = _lib.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_bundle_adjustment"] == (i, [vp] * 5)
    assert protos["orbm_ba_plan"] == (i, [vp] * 8)
    assert protos["orbm_debug_last_ba_waits"] == (i, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for fn in ("orbm_bundle_adjustment", "orbm_ba_plan", "orbm_debug_last_ba_waits"):
        assert f" T {fn}\n" in out, fn
    assert _lib.lib().orbx_abi_version() == 136


def test_struct_mirrors_and_initialisers_have_the_c_values(tmp_path):
    exe = str(tmp_path / "abi_layout_ba")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_ba.c"), "-o", exe])
    sizes, fields, opts = {}, {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        elif w[0] == "field":
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
        else:
            opts[w[1]] = [float(x) for x in w[2:]]
    for m, name in ((bundle.BaGraph, "orbm_ba_graph"), (bundle.BaOptions, "orbm_ba_options"), (bundle.BaResult, "orbm_ba_result"),
                    (bundle.BaStats, "orbm_ba_stats"), (ba_oracle.Graph, "orbm_ba_graph"), (ba_oracle.Options, "orbm_ba_options")):
        assert C.sizeof(m) == sizes[name], name
        assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name], name
    for d in (bundle.BA_TRIAL_DTYPE, ba_oracle.TRIAL_DTYPE):
        assert d.itemsize == sizes["orbm_ba_trial"]
        assert [(d.fields[n][1], d.fields[n][0].itemsize) for n in d.names] == [(o, w) for _, o, w in fields["orbm_ba_trial"]]

    def values(o):
        return [o.nrounds, o.iterations[0], o.iterations[1], o.robust_round0, o.classify, o.huber_mono, o.huber_stereo, o.chi2_mono, o.chi2_stereo]
    assert values(bundle.local_options()) == opts["local"]
    assert values(bundle.global_options(20, False)) == opts["global"]
    # the deltas are the reference's FLOATS: thHuber2D = sqrt(5.99) in BundleAdjustment, sqrt(5.991) in LocalBundleAdjustment
    assert opts["local"][5] == float(np.float32(np.sqrt(5.991))) != opts["global"][5] == float(np.float32(np.sqrt(5.99)))
    assert opts["local"][6] == opts["global"][6] == float(np.float32(np.sqrt(7.815)))
    assert (opts["local"][7], opts["global"][7], opts["local"][8]) == (5.991, 5.99, 7.815)


# ------------------------------------------------------------------------------------------------ 2. the host planning
def _numpy_plan(g):
    nfree, npose, npts = g["nfree"], len(g["poses"]), len(g["points"])
    ep, ec = g["e_point"], g["e_cam"]
    pose_class = np.full(npose, 2, np.int32); pose_class[nfree:] = 1
    pose_class[np.unique(ec)] = 0
    pose_class[nfree:] = 1
    if g["fixed"] is not None:
        pose_class[:nfree][g["fixed"] != 0] = 1
    point_class = np.ones(npts, np.int32); point_class[np.unique(ep)] = 0
    free = pose_class[:nfree] == 0
    pose_edges = [np.nonzero(ec == p)[0] if free[p] else np.zeros(0, np.int64) for p in range(nfree)]
    blocks = {}
    for n in np.unique(ep):
        es = [e for e in np.nonzero(ep == n)[0] if ec[e] < nfree and free[ec[e]]]
        for a in es:
            for b in es:
                if ec[a] <= ec[b]:
                    blocks.setdefault((int(ec[a]), int(ec[b])), []).append((int(n), int(a), int(b)))
    return pose_class, point_class, pose_edges, blocks


@pytest.mark.parametrize("name", ["baseline", "nfree1", "nfree11", "kf0_fixed", "fixed_plus_one", "global_robust", "multi_block"])
def test_plan_gives_the_lists_built_in_numpy(name, scenes):
    g = next(g for n, g, _ in scenes if n == name)
    p = bundle.plan(g)
    pose_class, point_class, pose_edges, blocks = _numpy_plan(g)
    nfree = g["nfree"]
    assert np.array_equal(p["pose_class"], pose_class) and np.array_equal(p["point_class"], point_class)
    for k in range(nfree):
        assert np.array_equal(p["pose_edges"][p["pose_edge_start"][k]:p["pose_edge_start"][k + 1]], pose_edges[k]), k
    assert p["pose_edge_start"][nfree] == len(p["pose_edges"]) == sum(len(e) for e in pose_edges)
    b = 0
    for i1 in range(nfree):
        for i2 in range(i1, nfree):
            assert b == i1 * nfree - i1 * (i1 - 1) // 2 + i2 - i1
            got = p["block_entries"][p["block_start"][b]:p["block_start"][b + 1]]
            assert got.tolist() == [list(t) for t in blocks.get((i1, i2), [])], (i1, i2)
            assert (np.diff(got[:, 0]) > 0).all()                                   # points ascending, each once
            b += 1
    assert p["block_start"][b] == len(p["block_entries"])
    if name == "kf0_fixed":
        assert p["pose_class"][0] == 1 and p["pose_edge_start"][1] == 0             # the local keyframe with id 0: fixed, no list
    if name == "global_robust":
        assert p["point_class"][-2:].tolist() == [1, 1]                             # the points without edges


# ------------------------------------------------------------------------------------------------ 3. refusals
def _call(g, opt, sizes=None, null=(), stats=False):
    """orbm_bundle_adjustment with sentinel-filled outputs; returns (rc, outputs untouched)"""
    L = _lib.lib()
    cg = bundle.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    for k in null:
        setattr(cg, k, None)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    poses = np.full((nfree + 70, 16), 7.5, np.float32); points = np.full((npts + 1, 3), 7.5, np.float32)
    erase = np.full(ne + 1, 77, np.uint8); notinc = np.full(npts + 1, 77, np.uint8)
    res = bundle.BaResult(bundle.ptr(poses), bundle.ptr(points), bundle.ptr(erase), bundle.ptr(notinc), 77)
    rc = L.orbm_bundle_adjustment(C.byref(cg), C.byref(opt), None, C.byref(res), None)
    untouched = (poses == 7.5).all() and (points == 7.5).all() and (erase == 77).all() and (notinc == 77).all() and res.stopped == 77
    return rc, bool(untouched)


def test_every_refusal_comes_before_any_device_work_and_writes_nothing(scenes):
    g = next(g for n, g, _ in scenes if n == "baseline")
    opt = bundle.local_options()
    for sizes in ({"nfree": 65}, {"nfixed": 1025}, {"npoints": 65537}, {"nedges": 524289}):
        assert _call(g, opt, sizes) == (ERR_UNSUPPORTED, True), sizes
    for sizes in ({"nfree": -1}, {"nfixed": -1}, {"npoints": -1}, {"nedges": -1}):
        assert _call(g, opt, sizes) == (ERR_ARG, True), sizes
    for null in ("poses", "points", "e_point", "e_cam", "e_obs", "e_inv_sigma2", "e_cam_k"):
        assert _call(g, opt, null=(null,)) == (ERR_ARG, True), null

    def edited(**kw):
        h = dict(g)
        for k, v in kw.items():
            h[k] = v
        return h
    ep, ec = g["e_point"], g["e_cam"]
    swapped = ep.copy(); swapped[[0, len(ep) - 1]] = swapped[[len(ep) - 1, 0]]
    assert _call(edited(e_point=swapped), opt) == (ERR_ARG, True)                       # not grouped by ascending point
    for bad in (-1, len(g["points"])):
        e = ep.copy(); e[-1] = bad
        assert _call(edited(e_point=e), opt) == (ERR_ARG, True)
    for bad in (-1, len(g["poses"])):
        e = ec.copy(); e[3] = bad
        assert _call(edited(e_cam=e), opt) == (ERR_ARG, True)
    twice = ec.copy(); twice[1] = twice[0]
    assert ep[0] == ep[1]
    assert _call(edited(e_cam=twice), opt) == (ERR_ARG, True)                           # a keyframe observes a point twice
    assert b"twice" in _lib.lib().orbx_last_error()
    for field, value in (("nrounds", 0), ("nrounds", 3), ("robust_round0", 2), ("classify", -1), ("huber_mono", 0.0), ("huber_stereo", -1.0),
                         ("chi2_mono", float("nan")), ("chi2_stereo", float("inf"))):
        o = bundle.local_options(); setattr(o, field, value)
        assert _call(g, o) == (ERR_ARG, True), field
    o = bundle.local_options(); o.iterations[1] = 65
    assert _call(g, o) == (ERR_ARG, True)
    # the planning entry refuses the same graphs
    cg = bundle.c_graph(g); cg.nfree = 65
    assert _lib.lib().orbm_ba_plan(C.byref(cg), None, None, None, None, None, None, None) == ERR_UNSUPPORTED


def test_degenerate_graphs_return_the_input_without_a_launch(scenes):
    g = next(g for n, g, _ in scenes if n == "global_robust")
    none = dict(g); none.update(e_point=g["e_point"][:0], e_cam=g["e_cam"][:0], e_obs=g["e_obs"][:0], e_inv_sigma2=g["e_inv_sigma2"][:0],
                                e_cam_k=g["e_cam_k"][:0])
    r = bundle.run(none, bundle.global_options(5, True), want_stats=True)
    assert np.array_equal(r["poses"], g["poses"][:g["nfree"]]) and np.array_equal(r["points"], g["points"]) and r["not_included"].all()
    assert r["waits"] == 0 and r["ntrials"] == 0 and r["stopped"] == 0
    nofree = dict(g); nofree["nfree"] = 0; nofree["fixed"] = None
    r = bundle.run(nofree, bundle.local_options())
    assert np.array_equal(r["points"], g["points"]) and r["waits"] == 0 and not r["erase"].any()
    # the stop flag set before the first optimize (Optimizer.cc:1039-1041): nothing changes, nothing is launched
    r = bundle.run(g, bundle.local_options(), stop_flag=np.ones(1, np.uint8), want_stats=True)
    assert r["stopped"] == 1 and r["waits"] == 0 and np.array_equal(r["poses"], g["poses"][:g["nfree"]]) and np.array_equal(r["points"], g["points"])


# ------------------------------------------------------------------------------------------------ 4. known answers of the restatement
def test_zero_noise_gives_no_update_and_no_erase():
    """Exact observations, exact start: what is left is the rounding of the inputs to float (6e-8 relative: 3e-5 px at 517 px), so
    the estimates move by less than 1e-5 of their size and nothing is erased."""
    g = ba_scenes.make(nfree=3, nfixed=2, npoints=30, seed=7, noise_px=0.0, pose_err=(0.0, 0.0), point_err=0.0)
    r = ba_oracle.run(g, bundle.local_options())
    assert np.abs(r["poses"] - g["poses"][:3]).max() <= 1e-5 * np.abs(g["poses"]).max()
    assert np.abs(r["points"] - g["points"]).max() <= 1e-5 * np.abs(g["points"]).max()
    assert not r["erase"].any() and not r["level"].any() and r["chi2"].max() < 1e-4


def test_planted_entries_do_what_their_scene_says(scenes, reference):
    by = {n: (g, o) for n, g, o in scenes}
    g, _ = by["outlier"]; r = reference["outlier"]
    assert np.nonzero(r["level"])[0].tolist() == g["planted"] == np.nonzero(r["erase"])[0].tolist()     # level 1 after round 0, erased
    g, _ = by["behind"]; r = reference["behind"]
    n = len(g["points"]) - 1
    _, depth = ba_optimum.edge_chi2(g, r["poses_d"], r["points_d"])
    e = np.nonzero((g["e_point"] == n) & (g["e_cam"] == 0))[0][0]
    assert depth[e] < 0 and r["erase"][e]                                                                # behind its camera at the end
    g, _ = by["keyframe_drops_out"]; r = reference["keyframe_drops_out"]
    k = g["nfree"] - 1
    assert r["level"][g["e_cam"] == k].all() and (g["e_cam"] == k).sum() >= 3                            # the keyframe left round 2 ...
    start = ba_oracle.run(g, bundle.BaOptions(1, (5, 0), 1, 1, 0, *[getattr(bundle.local_options(), f) for f in
                                                                     ("huber_mono", "huber_stereo", "chi2_mono", "chi2_stereo")]))
    assert np.array_equal(start["poses_d"][k], r["poses_d"][k])                                          # ... and kept round 0's estimate
    assert not np.array_equal(start["poses_d"][0], r["poses_d"][0])
    g, _ = by["point_drops_out"]; r = reference["point_drops_out"]
    assert r["level"][g["e_point"] == 1].all() and np.array_equal(start_point(g, 1), r["points_d"][1])
    g, _ = by["single_mono"]; r = reference["single_mono"]
    assert (g["e_point"] == len(g["points"]) - 1).sum() == 1 and g["e_obs"][g["e_point"] == len(g["points"]) - 1, 2] < 0
    assert np.isfinite(r["points_d"]).all()                                                              # rank-2 Hll, regular through lambda
    g, _ = by["fixed_plus_one"]
    n = len(g["points"]) - 1
    assert sorted(g["e_cam"][g["e_point"] == n].tolist()) == [0, 2, 3] and g["nfree"] == 2
    g, _ = by["global_robust"]; r = reference["global_robust"]
    assert r["not_included"].tolist() == [0] * 30 + [1, 1] and np.array_equal(r["points"][-2:], g["points"][-2:]) and r["rounds"] == 1
    assert np.abs(r["poses"][0] - g["poses"][0]).max() <= 1e-6                                           # the fixed keyframe 0: a round trip
    assert reference["global_plain"]["trials"] != r["trials"]                                            # bRobust changes the run


def start_point(g, n):
    """point n after round 0 alone"""
    lo = bundle.local_options()
    return ba_oracle.run(g, bundle.BaOptions(1, (5, 0), 1, 1, 0, lo.huber_mono, lo.huber_stereo, lo.chi2_mono, lo.chi2_stereo))["points_d"][n]


def test_first_trial_is_the_damped_gauss_newton_step_of_a_numpy_model(scenes, reference):
    """global_plain (no robust kernel): computeLambdaInit and the first trial's chi2 against a dense numpy model with central-difference
    Jacobians and plain double projection.  The stereo edges' float invz (6e-8 relative in the projection) is the difference."""
    g = next(g for n, g, _ in scenes if n == "global_plain")
    lam, c0, c1 = ba_optimum.first_trial_chi2(g)
    r = reference["global_plain"]
    assert abs(lam - r["lambda_init"][0]) <= 1e-7 * lam                 # measured 1.0e-8
    assert abs(c1 - r["trial_log"]["tempChi"][0]) <= 9.2e-6 * c1        # measured 9.2e-7
    assert c1 < c0


@pytest.mark.parametrize("k", [3, 5])
def test_next_trial_is_the_damped_gauss_newton_step_with_the_last_lambda(k, scenes):
    """global_plain after optimize(k): one damped Gauss-Newton step of the numpy model from the RETURNED estimates with the LAST
    lambda lands on the tempChi of the trial that optimize(k + 1) runs next.  Measured on the restatement: 3.1e-7 (k = 3), 1.1e-6
    (k = 5); the float invz of the stereo edges is the difference.  tests/test_gpu_ba.py holds the device to 10 times the larger."""
    g = next(g for n, g, _ in scenes if n == "global_plain")
    A = ba_oracle.run(g, bundle.global_options(k, False)); B = ba_oracle.run(g, bundle.global_options(k + 1, False))
    la = A["trial_log"]
    assert la["accepted"][-1] == 1 and A["results"][-1] == 1 and B["ntrials"] > A["ntrials"]
    _, c0, c1 = ba_optimum.next_trial_chi2(g, A["poses_d"], A["points_d"], la["lam"][-1])
    nxt = B["trial_log"][A["ntrials"]]
    assert nxt["qmax"] == 0 and abs(c1 - nxt["tempChi"]) <= 1.1e-5 * c1 and c1 < c0


def test_stored_error_of_a_rejected_last_trial_decides_the_final_pass(scenes):
    """chi2() reads the STORED error.  The stop flag, read in the trial loop's condition, ends an iteration behind a rejected trial: the
    estimates are popped, the stored errors are the rejected estimate's, there is no second round and the final pass uses them."""
    found = 0
    lo = bundle.local_options()
    # optimize(20) in the first round: the scenes' rejected trials come behind the fifth iteration
    opt = bundle.BaOptions(2, (20, 10), 1, 1, 0, lo.huber_mono, lo.huber_stereo, lo.chi2_mono, lo.chi2_stereo)
    for name, g, _ in scenes:
        full = ba_oracle.run(g, opt)
        for k in range(2, full["nreads"] + 1):
            r = ba_oracle.run(g, opt, stop_at=k)
            log = r["trial_log"]
            if not len(log) or log["accepted"][-1] or r["rounds"] != 1:
                continue
            assert r["stopped"] == 2
            erase_now, chi2_now, th = ba_optimum.erase_list(g, opt, r["poses_d"], r["points_d"])
            assert np.abs(r["chi2"] - chi2_now).max() > 1e-6 * chi2_now.max()                   # stale: not the restored estimate's
            _, depth = ba_optimum.edge_chi2(g, r["poses_d"], r["points_d"])
            assert np.array_equal(r["erase"], ((r["chi2"] > th) | ~(depth > 0)).astype(np.uint8))
            found += 1
            break
    assert found >= 1


def test_a_round_that_ends_on_rejected_trials_ends_at_the_rounding_floor():
    """Why tests/ba_scenes.py holds no scene whose first round ends on a rejected trial WITHOUT the stop flag.  The trial loop ends
    behind a rejection only at qmax == 10 (or at a rho that is 0 or NaN).  Ten rejections in a row multiply lambda by 2, 4, 8, ...:
    2^45 by the tenth trial, so the tenth step is 3e-14 of the first, and its rho -- the change of chi2 over a scale that is 1e-3
    at the least -- is far below the 1e-9 under which a trial's sign belongs to rounding and the scene leaves the comparison
    (ba_compare.RHO_FLOOR).  The search: from well-separated starts (1,440 scenes: stereo and mixed edges, 0 / 0.05 / 0.5 px noise,
    three start errors, with and without an outlier, 40 seeds each) NO first round ends on a rejection; from converged starts
    (preconverged: 720 scenes over the three edge types, 2 noise levels, with and without an outlier, 60 seeds) 60 do, every one
    with a last |rho| below 1e-9 -- 0 inside the selection rule.  This test repeats a slice of the second search (mixed edges,
    0.5 px, 24 seeds) and holds it to that: hits exist, each ends with qmax == 10 or rho == 0, none has a last |rho| >= 1e-9.  The
    rejected step there is also 1e-13 of an ordinary one, so the stale stored error it leaves cannot decide an edge: only a
    rejection EARLY in a trial loop can, and only the stop flag ends the loop there
    (test_stored_error_of_a_rejected_last_trial_decides_the_final_pass)."""
    hits = 0
    for seed in range(7020, 7044):
        r = ba_oracle.run(ba_scenes.preconverged(seed), bundle.local_options())
        log = r["trial_log"]
        l0 = log[log["round"] == 0]
        if not len(l0) or l0["accepted"][-1]:
            continue
        hits += 1
        assert l0["qmax"][-1] == 9 or l0["rho"][-1] == 0, seed
        assert abs(l0["rho"][-1]) < ba_compare.RHO_FLOOR, seed
    assert hits >= 3


# ------------------------------------------------------------------------------------------------ 5. sensitivity and scene selection
def test_sensitivity_is_the_pinned_one_and_no_scene_decides_at_the_rounding_floor():
    D, rows = ba_compare.measure_sensitivity()
    floor = [r["name"] for r in rows if r["near"] or r["small_rho"] or r["moved"]]
    print("D_cpu %.3e" % D, "scenes:", len(rows), "at the floor:", floor)
    gold = json.load(open(ba_compare.GOLDEN))
    assert gold["scenes"] == [r["name"] for r in rows] and gold["ulp_seeds"] == ba_compare.ULP_SEEDS
    assert len(floor) <= ba_compare.CAP * len(rows), floor                 # 16 scenes: none may sit at the floor
    # the pinned figure: the same arithmetic on another libm may round sin / cos / pow differently, which is what D measures
    assert gold["D_cpu"] / 2 <= D <= gold["D_cpu"] * 2, (D, gold["D_cpu"])
    assert 1e-12 < gold["D_cpu"] < 1e-7
    # the entry-by-entry measures (stored chi2, lambda, the chi2 sums): pinned likewise; lambda follows rho's last bits most closely
    assert set(gold["D_each"]) == set(ba_compare.D_EACH) == {"chi2", "lambda", "tempChi", "currentChi"}
    for k, v in ba_compare.D_EACH.items():
        assert gold["D_each"][k] / 2 <= v <= gold["D_each"][k] * 2, (k, v, gold["D_each"][k])
        assert gold["D_each"][k] < 1e-6, k


def test_the_lease_site_has_its_stale_workspace_case():
    """orbm_ba.hip leases ONE pooled workspace; its stale-arena case is tests/test_gpu_ba_workspace.py, under every fill of the table."""
    import re
    src = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_ba.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*(?:\{\})?;", src, re.M)) == 1 and "WorkspaceLease" not in src
    case = open(os.path.join(ROOT, "tests", "test_gpu_ba_workspace.py")).read()
    assert "W.FILLS" in case and "fill_workspaces" in case and "bundle.run" in case


def test_integration_shell_calls_the_declared_entry_point_and_fills_every_field():
    """integration/Optimizer_ba_hip.cc cannot be compiled here (no OpenCV): its C-ABI call is declared with that many arguments and
    exported, it sets every member of the graph and of the result, takes both documented initialisers, and says what it leaves out."""
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    import re
    decl, header_text = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_ba_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert calls.count(("orbm_bundle_adjustment", 5)) == 2
    for fn, n in calls:
        assert decl[fn] == n and hasattr(_lib.lib(), fn), fn
    for f, _ in bundle.BaGraph._fields_:
        assert f"g.{f} =" in src, f
    for f, _ in bundle.BaResult._fields_:
        assert src.count(f"res.{f} = ") == 2, f
    assert "ORBM_BA_OPTIONS_LOCAL" in src and "ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust)" in src
    assert "mnId == 0" in src and "mTcwGBA" in src and "mPosGBA" in src and "UpdateNormalAndDepth" in src and "EraseObservation" in src
    assert "isBad()" in raw and "NOT reproduced" in raw
    for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert tok in header_text or tok in open(os.path.join(ROOT, "include", "orbslam_hip.h")).read(), tok


def test_integration_shell_leaves_no_marks_behind_a_refusal():
    """integration/Optimizer_ba_hip.cc: the reference's body runs behind `if (HipLocalBundleAdjustment(...)) return;` and tests the
    marks the walk sets (src/Optimizer.cc:864, :881).  The shell counts the local keyframes before anything is marked, sets every
    mark through the recorder, and undoes them on the one later `return false`."""
    from test_cpu_integration_shells import _strip_comments
    import re
    src = _strip_comments(open(os.path.join(ROOT, "integration", "Optimizer_ba_hip.cc")).read())
    body = src[src.index("bool HipLocalBundleAdjustment"):src.index("bool HipBundleAdjustment")]
    # no mark is written except through Mark::set (whose own assignment is `member = v`)
    assert not re.search(r"->mnBA(?:Local|Fixed)ForKF\s*=[^=]", body)
    assert body.count("Mark::set(marks,") == 4                                      # pKF, the neighbours, the points, the fixed keyframes
    first_mark = body.index("Mark::set(marks,")
    falses = [m.start() for m in re.finditer(r"return false;", body)]
    assert len(falses) == 2 and falses[0] < first_mark < falses[1]                  # the count refuses before any mark ...
    assert "nLocal > 64" in body[:first_mark]
    assert re.search(r"Mark::undo\(marks\);\s*return false;", body)                 # ... the later limits put them back
    # the global form's walk writes nothing before its call
    glob = src[src.index("bool HipBundleAdjustment"):]
    call = glob.index("orbm_bundle_adjustment(")
    assert not re.search(r"->\w+\s*=[^=]", glob[:call]) and "SetPose" not in glob[:call]
