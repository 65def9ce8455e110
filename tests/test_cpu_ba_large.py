"""orbm_global_bundle_adjustment / orbm_global_ba_plan, the part that needs no device: the scenes of tests/ba_large_scenes.py inside
the selection rule of tests/ba_compare.py against their own pinned sensitivity, the 512-keyframe golden made from the scene it says,
the new limits with every refusal before any device work and nothing written, the planning lists against numpy, and what the
sources must keep (one lease in orbm_ba.hip, none in orbm_llt.hip, the shell's one call of the new entry)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import ba_compare
import ba_large_scenes as LS
from orb_slam2_e_amd import _lib, bundle
from test_cpu_ba import _numpy_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5


# ------------------------------------------------------------------------------------------------ 1. the scenes and their goldens
def test_scenes_are_inside_the_selection_rule_and_the_sensitivity_is_the_pinned_one():
    """The restatement alone, on the scenes up to t130 (t200's 17 runs take too long for the suite; its row of the file is
    write_golden()'s): no integer moves under the 16 ulp patterns, no stored chi2 near its threshold, no trial with |rho| < 1e-9."""
    names = LS.MEASURED[:4]
    D, rows = ba_compare.measure_sensitivity(LS.scenes(names))
    floor = [r["name"] for r in rows if r["near"] or r["small_rho"] or r["moved"]]
    print("D_large %.3e" % D, {r["name"]: "%.3e" % r["d"] for r in rows}, "at the floor:", floor)
    gold = json.load(open(LS.GOLDEN))
    assert gold["scenes"] == LS.MEASURED == [s[0] for s in LS.SPECS[:5]] and gold["ulp_seeds"] == ba_compare.ULP_SEEDS
    assert len(floor) <= ba_compare.CAP * len(rows), floor                 # 2 % of 4 scenes: none
    for r in rows:                                                          # another libm may round sin / cos / pow differently
        assert gold["d"][r["name"]] / 4 <= r["d"] <= gold["d"][r["name"]] * 4, (r["name"], r["d"], gold["d"][r["name"]])
    assert gold["D_cpu"] == max(gold["d"].values()) and 1e-16 < gold["D_cpu"] < 1e-7
    assert set(gold["D_each"]) == {"chi2", "lambda", "tempChi", "currentChi"} and all(v < 1e-6 for v in gold["D_each"].values())
    by = {r["name"]: r["base"] for r in rows}
    assert by["t65_local"]["rounds"] == 2 and by["t96_global"]["rounds"] == 1 and by["t96_global"]["not_included"][-2:].all()
    g = LS.scene("t70_drop")[1]
    assert by["t70_drop"]["level"][g["e_cam"] == g["nfree"] - 1].all()     # the keyframe leaves the second round's system


def test_scene_sizes_are_the_ones_the_names_say():
    for name, nfree, nfixed, npts in (("t65_local", 65, 2, 330), ("t70_drop", 70, 1, 350), ("t96_global", 96, 0, 482), ("t130_global_robust", 130, 0, 650),
                                      ("t200_global", 200, 0, 1000), ("t512_global", 512, 0, 2500)):
        _, g, opt = LS.scene(name)
        assert (g["nfree"], len(g["poses"]) - g["nfree"], len(g["points"])) == (nfree, nfixed, npts), name
        assert opt.nrounds == (2 if nfixed else 1) and (nfixed or g["fixed"][0] == 1), name


def test_the_512_golden_was_made_from_the_scene():
    gold, sha = LS.load_512()
    _, g, opt = LS.scene("t512_global")
    assert sha == LS.input_hash(g)
    assert gold["poses_d"].shape == (512, 7) and gold["points_d"].shape == (2500, 3) and len(gold["chi2"]) == len(g["e_point"])
    log = gold["trial_log"]
    assert gold["trials"] == [5, 0] and log["accepted"].all() and (np.abs(log["rho"]) > 0.9).all() and gold["rounds"] == 1
    assert os.path.getsize(LS.GOLDEN_512) < 400 * 1024


# ------------------------------------------------------------------------------------------------ 2. limits and refusals
def _call(g, opt, sizes=None, null=()):
    """orbm_global_bundle_adjustment with sentinel-filled outputs; returns (rc, outputs untouched)"""
    L = _lib.lib()
    cg = bundle.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    for k in null:
        setattr(cg, k, None)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    poses = np.full((nfree + 520, 16), 7.5, np.float32); points = np.full((npts + 1, 3), 7.5, np.float32)
    erase = np.full(ne + 1, 77, np.uint8); notinc = np.full(npts + 1, 77, np.uint8)
    res = bundle.BaResult(bundle.ptr(poses), bundle.ptr(points), bundle.ptr(erase), bundle.ptr(notinc), 77)
    rc = L.orbm_global_bundle_adjustment(C.byref(cg), C.byref(opt), None, C.byref(res), None)
    untouched = (poses == 7.5).all() and (points == 7.5).all() and (erase == 77).all() and (notinc == 77).all() and res.stopped == 77
    return rc, bool(untouched)


def test_512_keyframes_are_planned_and_513_refused():
    _, g, _ = LS.scene("t512_global")
    p = bundle.plan_global(g)
    assert len(p["block_start"]) == 512 * 513 // 2 + 1 and p["block_start"][-1] == len(p["block_entries"]) > 0
    assert p["pose_class"].tolist() == [1] + [0] * 511
    L = _lib.lib()
    for entry in (L.orbm_global_ba_plan, L.orbm_ba_plan):
        cg = bundle.c_graph(g); cg.nfree = 513
        assert entry(C.byref(cg), None, None, None, None, None, None, None) == ERR_UNSUPPORTED
    assert _call(g, bundle.global_options(10, False), {"nfree": 513}) == (ERR_UNSUPPORTED, True)
    assert b"512" in L.orbx_last_error()
    # the other entry keeps its own limit
    cg = bundle.c_graph(LS.scene("t65_local")[1])
    assert L.orbm_ba_plan(C.byref(cg), None, None, None, None, None, None, None) == ERR_UNSUPPORTED
    assert L.orbm_global_ba_plan(C.byref(cg), None, None, None, None, None, None, None) == OK


def test_every_refusal_comes_before_any_device_work_and_writes_nothing():
    """the list of tests/test_cpu_ba.py::test_every_refusal_comes_before_any_device_work_and_writes_nothing, for the new entry"""
    _, g, _ = LS.scene("t65_local")
    opt = bundle.local_options()
    for sizes in ({"nfree": 513}, {"nfixed": 1025}, {"npoints": 65537}, {"nedges": 524289}):
        assert _call(g, opt, sizes) == (ERR_UNSUPPORTED, True), sizes
    for sizes in ({"nfree": -1}, {"nfixed": -1}, {"npoints": -1}, {"nedges": -1}):
        assert _call(g, opt, sizes) == (ERR_ARG, True), sizes
    for null in ("poses", "points", "e_point", "e_cam", "e_obs", "e_inv_sigma2", "e_cam_k"):
        assert _call(g, opt, null=(null,)) == (ERR_ARG, True), null

    def edited(**kw):
        h = dict(g)
        h.update(kw)
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
    L = _lib.lib()
    assert L.orbm_global_bundle_adjustment(None, C.byref(opt), None, None, None) == ERR_ARG
    assert L.orbm_global_ba_plan(None, None, None, None, None, None, None, None) == ERR_ARG


def test_the_block_entry_cap_is_refused_before_the_lists_are_built():
    """256 points seen by all 512 keyframes: 256 x 512 x 513 / 2 = 33,619,968 block entries, above 2^25 = 33,554,432 (a list of 403 MB)
    with only 131,072 edges.  Both new entries refuse it with nothing written; the old entry's worst case, 8,192 points seen by all 64
    keyframes (524,288 edges), is 17,039,360 entries and below the cap, so no graph it admits is refused for this."""
    assert 256 * 512 * 513 // 2 > 2 ** 25 >= 255 * 512 * 513 // 2 and 8192 * 64 * 65 // 2 < 2 ** 25
    nk, npts = 512, 256
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), (nk, 1))
    ne = nk * npts
    g = bundle.make_graph(poses, nk, np.zeros((npts, 3)), np.repeat(np.arange(npts), nk), np.tile(np.arange(nk), npts), np.ones((ne, 3)),
                          np.ones(ne), np.ones((ne, 5)))
    assert _call(g, bundle.global_options(10, False)) == (ERR_UNSUPPORTED, True)
    assert b"2^25" in _lib.lib().orbx_last_error()
    counts = np.full(2, -7, np.int32)
    cg = bundle.c_graph(g)
    assert _lib.lib().orbm_global_ba_plan(C.byref(cg), None, None, None, None, None, None, bundle.ptr(counts)) == ERR_UNSUPPORTED
    assert counts.tolist() == [-7, -7]
    # one point fewer per keyframe pair is inside it: the same pattern with 64 points is planned (8,404,992 entries)
    small = bundle.make_graph(poses, nk, np.zeros((64, 3)), np.repeat(np.arange(64), nk), np.tile(np.arange(nk), 64), np.ones((64 * nk, 3)),
                              np.ones(64 * nk), np.ones((64 * nk, 5)))
    cs = bundle.c_graph(small)
    assert _lib.lib().orbm_global_ba_plan(C.byref(cs), None, None, None, None, None, None, bundle.ptr(counts)) == OK
    assert counts.tolist() == [64 * nk, 64 * nk * (nk + 1) // 2]


# ------------------------------------------------------------------------------------------------ 3. the host planning
@pytest.mark.parametrize("name", ["t65_local", "t130_global_robust"])
def test_plan_global_gives_the_lists_built_in_numpy(name):
    _, g, _ = LS.scene(name)
    p = bundle.plan_global(g)
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
            b += 1
    assert p["block_start"][b] == len(p["block_entries"]) == sum(len(v) for v in blocks.values())
    if name == "t130_global_robust":
        assert p["pose_class"][0] == 1 and p["pose_edge_start"][1] == 0                 # keyframe 0: fixed, no list


def test_plan_global_equals_plan_where_both_accept_the_graph():
    import ba_scenes
    for name, g, _ in ba_scenes.scenes(["nfree11", "nfree64", "global_robust"]):
        a, b = bundle.plan(g), bundle.plan_global(g)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), name


# ------------------------------------------------------------------------------------------------ 4. the sources
def test_one_lease_in_the_ba_unit_and_none_in_the_solver():
    csrc = os.path.join(ROOT, "orb_slam2_e_amd", "csrc")
    ba = open(os.path.join(csrc, "orbm_ba.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*(?:\{\})?;", ba, re.M)) == 1 and "WorkspaceLease" not in ba
    assert ba.count("k_ba_solve, dim3(1), dim3(ST)") == 1 and ba.count("orbm_llt_solve_dev(") == 1      # one body, either solver
    llt = open(os.path.join(csrc, "orbm_llt.hip")).read()
    assert "StagedCall" not in llt and "WorkspaceLease" not in llt
    case = open(os.path.join(ROOT, "tests", "test_gpu_ba_large.py")).read()
    assert "W.FILLS" in case and "fill_workspaces" in case and "bundle.run_global" in case


def test_integration_shell_takes_the_new_entry_above_64_keyframes():
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, _ = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_ba_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert calls.count(("orbm_global_bundle_adjustment", 5)) == 1 and calls.count(("orbm_bundle_adjustment", 5)) == 2
    assert decl["orbm_global_bundle_adjustment"] == 5 and hasattr(_lib.lib(), "orbm_global_bundle_adjustment")
    glob = src[src.index("bool HipBundleAdjustment"):]
    assert re.search(r"rc\s*=\s*nfree\s*>\s*64\s*\?\s*orbm_global_bundle_adjustment\(.*?\)\s*:\s*orbm_bundle_adjustment\(", glob, re.S)
    # beyond 512 keyframes: false, before the call and before anything is written to a keyframe or a point
    refuse = glob.index("> 512) return false;")
    assert refuse < glob.index("orbm_global_bundle_adjustment(")
    assert not re.search(r"->\w+\s*=[^=]", glob[:refuse]) and "SetPose" not in glob[:refuse] and "SetWorldPos" not in glob[:refuse]
    # the local form is unchanged: it never takes the new entry
    local = src[src.index("bool HipLocalBundleAdjustment"):src.index("bool HipBundleAdjustment")]
    assert "orbm_global_bundle_adjustment" not in local and "nLocal > 64" in local
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    assert re.search(r"bool GlobalMap\(int nIterations, bool bRobust, const volatile uint8_t \*pbStopFlag = nullptr, orbm_ba_stats \*stats = nullptr\)", hpp)
