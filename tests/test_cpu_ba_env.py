"""orbm_global_bundle_adjustment_env / orbm_global_ba_env_plan, the part that needs no device: the compact block list
against orbm_global_ba_plan's dense one, the envelope against numpy and against orbm_llt_env_plan, the limits by plan alone, every
refusal before any device work with nothing written, the scenes of tests/ba_env_scenes.py inside the selection rule of
tests/ba_compare.py against their own pinned sensitivity, the e520 golden made from the scene it says, and what the sources must
keep (the new shell's one call, its sort before its numbering, its refusals before any write)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import ba_compare
import ba_env_scenes as ES
import ba_large_scenes as LS
from orb_slam2_e_amd import _lib, bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
PLANNED = [(n, "large") for n in (s[0] for s in LS.SPECS)] + [(n, "env") for n in ES.MEASURED]


def _graph(name, where):
    return (LS.scene(name) if where == "large" else ES.scene(name))[1]


def _rows(p, nfree):
    free = p["pose_class"][:nfree] == 0
    ridx = np.cumsum(free) - 1
    ridx[~free] = -1
    return ridx


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("name,where", PLANNED, ids=[n for n, _ in PLANNED])
def test_compact_lists_expanded_equal_the_dense_lists(name, where):
    g = _graph(name, where)
    nfree = g["nfree"]
    dense, p = bundle.plan_global(g), bundle.plan_global_env(g)
    for k in ("pose_class", "point_class", "pose_edge_start", "pose_edges"):
        assert np.array_equal(dense[k], p[k]), k
    i1, i2 = p["blk_i1"].astype(np.int64), p["blk_i2"].astype(np.int64)
    assert (i1 <= i2).all() and (np.diff(i1 * nfree + i2) > 0).all()                 # sorted by (i1, i2), no block twice
    index = i1 * nfree - i1 * (i1 - 1) // 2 + i2 - i1                               # the dense plan's block index
    start = np.zeros(nfree * (nfree + 1) // 2 + 1, np.int64)
    start[index + 1] = np.diff(p["block_start"])
    assert (np.diff(p["block_start"]) > 0).all()                                    # only non-empty blocks are listed
    assert np.array_equal(np.cumsum(start), dense["block_start"])
    assert np.array_equal(p["block_entries"], dense["block_entries"])               # the concatenation, empty blocks left out
    connected = np.nonzero(p["pose_class"][:nfree] == 0)[0]
    diag = set(i1[i1 == i2].tolist())
    assert diag == set(connected.tolist())                                          # every free, connected keyframe has its diagonal block
    for b in np.nonzero(i1 == i2)[0][:8]:                                           # ... whose entries are the pose's edge list, one for one
        k = i1[b]
        ent = p["block_entries"][p["block_start"][b]:p["block_start"][b + 1]]
        assert np.array_equal(ent[:, 1], p["pose_edges"][p["pose_edge_start"][k]:p["pose_edge_start"][k + 1]]) and np.array_equal(ent[:, 1], ent[:, 2])


@pytest.mark.parametrize("name,where", PLANNED + [("e70_drop", "env"), ("e65_shuffled", "env"), ("e520", "env")],
                         ids=[n for n, _ in PLANNED] + ["e70_drop", "e65_shuffled", "e520"])
def test_envelope_is_the_one_numpy_derives_from_the_block_list(name, where):
    g = _graph(name, where)
    p = bundle.plan_global_env(g)
    T = bundle.llt_tile()
    ridx = _rows(p, g["nfree"])
    first = ES.numpy_envelope(p["blk_i1"], p["blk_i2"], ridx, T)
    assert np.array_equal(p["first"], first)
    n = 6 * int((ridx >= 0).sum())
    solver = bundle.llt_env_plan(n, first)
    assert (p["live_tiles"], p["launches"]) == (solver["live_tiles"], solver["launches"])
    # ... and holds every non-zero of the system: entry (row, col) of a block lies in a live tile
    for b1, b2 in zip(p["blk_i1"], p["blk_i2"]):
        r1, r2 = ridx[b1], ridx[b2]
        for row, col in ((6 * r2, 6 * r1), (6 * r2 + 5, 6 * r1), (6 * r2 + 5, 6 * r1 + 5)):
            assert row < col or first[row // T] <= col // T


def test_what_the_scenes_are_there_for():
    T = bundle.llt_tile()
    assert T == 64
    sizes = {n: 6 * (ES.scene(n)[1]["nfree"] - 1) for n in ("e12", "e33_band", "e65_loop", "e65_shuffled")}
    assert sizes == {"e12": 66, "e33_band": 192, "e65_loop": 384, "e65_shuffled": 384}
    p = {n: bundle.plan_global_env(ES.scene(n)[1]) for n in ("e12", "e33_band", "e65_loop", "e130_robust", "e65_shuffled", "e520")}
    assert p["e12"]["first"].tolist() == [0, 0]                                      # two tiles, the last with two rows
    assert ((p["e12"]["blk_i2"] == 11) & (p["e12"]["blk_i1"] < 11)).any()            # keyframe 11 = rows 60 .. 65: a block straddles the edge
    assert len(p["e33_band"]["first"]) == 3 and p["e33_band"]["first"][2] == 1       # a band: the last row tile does not reach the first
    assert p["e65_loop"]["first"].tolist() == [0, 0, 1, 2, 3, 0]                     # the arrow: the loop reaches back from the last rows
    f = p["e130_robust"]["first"]
    assert (np.diff(f) < 0).any() and f[6] < f[5] and f[7] > f[6]                    # not monotone: the rows behind the loop start at their neighbour again
    assert p["e65_shuffled"]["live_tiles"] > p["e65_loop"]["live_tiles"]
    assert len(p["e520"]["first"]) == (6 * 519 + T - 1) // T and 6 * 519 % T != 0    # last tile partial
    assert ES.scene("e70_drop")[2].nrounds == 2 and ES.scene("e130_robust")[2].robust_round0 == 1


# ------------------------------------------------------------------------------------------------ 2. limits and refusals
def _plan_rc(g, sizes=None):
    L = _lib.lib()
    cg = bundle.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    counts = np.full(6, -7, np.int32)
    rc = L.orbm_global_ba_env_plan(C.byref(cg), *([None] * 9), bundle.ptr(counts))
    return rc, counts.tolist()


def _call(g, opt, sizes=None, null=()):
    """orbm_global_bundle_adjustment_env with sentinel-filled outputs; returns (rc, outputs untouched)"""
    L = _lib.lib()
    cg = bundle.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    for k in null:
        setattr(cg, k, None)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    poses = np.full((nfree + 8, 16), 7.5, np.float32); points = np.full((npts + 1, 3), 7.5, np.float32)
    erase = np.full(ne + 1, 77, np.uint8); notinc = np.full(npts + 1, 77, np.uint8)
    res = bundle.BaResult(bundle.ptr(poses), bundle.ptr(points), bundle.ptr(erase), bundle.ptr(notinc), 77)
    rc = L.orbm_global_bundle_adjustment_env(C.byref(cg), C.byref(opt), None, C.byref(res), None)
    untouched = (poses == 7.5).all() and (points == 7.5).all() and (erase == 77).all() and (notinc == 77).all() and res.stopped == 77
    return rc, bool(untouched)


def _chain(nk, extra=0):
    """nk keyframes, keyframe k and k + 1 share one point; `extra` keyframes more without an edge"""
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), (nk + extra, 1))
    npts = nk - 1
    ep = np.repeat(np.arange(npts), 2)
    ec = np.column_stack([np.arange(npts), np.arange(npts) + 1]).reshape(-1)
    return bundle.make_graph(poses, nk + extra, np.zeros((npts, 3)), ep, ec, np.ones((2 * npts, 3)), np.ones(2 * npts), np.ones((2 * npts, 5)))


def test_4096_keyframes_are_planned_and_4097_refused():
    g = _chain(4096)
    p = bundle.plan_global_env(g)
    T = bundle.llt_tile()
    assert len(p["first"]) == 6 * 4096 // T == 384 and p["live_tiles"] == 384 + 383 and len(p["blk_i1"]) == 4096 + 4095
    assert _plan_rc(_chain(4097)) == (ERR_UNSUPPORTED, [-7] * 6)
    assert b"4,096" in _lib.lib().orbx_last_error()
    assert _call(_chain(4097), bundle.global_options(10, False)) == (ERR_UNSUPPORTED, True)
    # the other entries keep their limits
    cg = bundle.c_graph(_chain(513))
    assert _lib.lib().orbm_global_ba_plan(C.byref(cg), None, None, None, None, None, None, None) == ERR_UNSUPPORTED
    assert _plan_rc(_chain(513))[0] == OK


def test_each_further_limit_has_its_own_refusal_with_nothing_written():
    _, g, opt = ES.scene("e65_loop")
    for sizes, text in (({"nfree": 4097}, b"4,096"), ({"nfixed": 1025}, b"1,024"), ({"npoints": (1 << 20) + 1}, b"1,048,576"),
                        ({"nedges": (1 << 22) + 1}, b"4,194,304")):
        assert _plan_rc(g, sizes) == (ERR_UNSUPPORTED, [-7] * 6), sizes
        assert text in _lib.lib().orbx_last_error(), sizes
        assert _call(g, opt, sizes) == (ERR_UNSUPPORTED, True), sizes
    for sizes in ({"nfree": -1}, {"nfixed": -1}, {"npoints": -1}, {"nedges": -1}):
        assert _call(g, opt, sizes) == (ERR_ARG, True), sizes
    for null in ("poses", "points", "e_point", "e_cam", "e_obs", "e_inv_sigma2", "e_cam_k"):
        assert _call(g, opt, null=(null,)) == (ERR_ARG, True), null
    o = bundle.global_options(65, False)
    assert _call(g, o) == (ERR_ARG, True)
    L = _lib.lib()
    assert L.orbm_global_bundle_adjustment_env(None, C.byref(opt), None, None, None) == ERR_ARG
    assert L.orbm_global_ba_env_plan(*([None] * 11)) == ERR_ARG


def test_the_block_entry_cap_is_refused_before_the_lists_are_built():
    """33 points seen by all 2,048 keyframes: 33 x 2,048 x 2,049 / 2 = 69,239,808 block entries, above 2^26 = 67,108,864, with only
    67,584 edges; 31 points are below it (and then refused for their full envelope of 18,528 tiles, the next check)."""
    assert 33 * 2048 * 2049 // 2 > 2 ** 26 > 31 * 2048 * 2049 // 2
    nk = 2048
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), (nk, 1))

    def full(npts):
        ne = nk * npts
        return bundle.make_graph(poses, nk, np.zeros((npts, 3)), np.repeat(np.arange(npts), nk), np.tile(np.arange(nk), npts), np.ones((ne, 3)),
                                 np.ones(ne), np.ones((ne, 5)))
    assert _plan_rc(full(33)) == (ERR_UNSUPPORTED, [-7] * 6)
    assert b"2^26" in _lib.lib().orbx_last_error()
    assert _call(full(33), bundle.global_options(10, False)) == (ERR_UNSUPPORTED, True)


def test_a_shuffled_band_is_refused_on_the_tile_cap():
    g = ES.wide_graph()
    assert g["nfree"] == 2048
    # by numpy alone: the envelope of the shuffled list has more than 8,192 live tiles (the same band in path order has a few hundred)
    T, nfree = bundle.llt_tile(), g["nfree"]
    fixed = int(np.nonzero(g["fixed"])[0][0])                                       # keyframe 0 of the PATH is fixed; where it is listed
    ridx = np.where(np.arange(nfree) < fixed, np.arange(nfree), np.arange(nfree) - 1); ridx[fixed] = -1
    pairs = set()
    ep, ec = g["e_point"], g["e_cam"]
    for n in np.unique(ep):
        cams = np.sort(ec[ep == n])
        pairs.update((a, b) for i, a in enumerate(cams) for b in cams[i:])
    first = ES.numpy_envelope([a for a, _ in pairs], [b for _, b in pairs], ridx, T)
    live = int((np.arange(len(first)) - first + 1).sum())
    assert live > 8192, live
    assert _plan_rc(g) == (ERR_UNSUPPORTED, [-7] * 6)
    assert b"8,192" in _lib.lib().orbx_last_error()
    assert _call(g, bundle.global_options(10, False)) == (ERR_UNSUPPORTED, True)
    ordered = bundle.plan_global_env(ES.make(nfree=2048, seed=509, w=4, points_per_kf=2))
    assert ordered["live_tiles"] < 600


# ------------------------------------------------------------------------------------------------ 3. the scenes and their goldens
def test_scenes_are_inside_the_selection_rule_and_the_sensitivity_is_the_pinned_one():
    """The restatement alone, on the scenes up to e130: no integer moves under the 16 ulp patterns, no stored chi2 near its threshold
    where classify is on, no trial with |rho| < 1e-9.  None is left out."""
    D, rows = ba_compare.measure_sensitivity(ES.scenes(ES.MEASURED))
    floor = [r["name"] for r in rows if r["near"] or r["small_rho"] or r["moved"]]
    print("D_env %.3e" % D, {r["name"]: "%.3e" % r["d"] for r in rows}, "at the floor:", floor)
    gold = json.load(open(ES.GOLDEN))
    assert gold["scenes"] == ES.MEASURED == ["e12", "e33_band", "e65_loop", "e130_robust"] and gold["ulp_seeds"] == ba_compare.ULP_SEEDS
    assert floor == []
    for r in rows:                                                          # another libm may round sin / cos / pow differently
        assert gold["d"][r["name"]] / 4 <= r["d"] <= gold["d"][r["name"]] * 4, (r["name"], r["d"], gold["d"][r["name"]])
    assert gold["D_env"] == max(gold["d"].values()) and 1e-16 < gold["D_env"] < 1e-7
    assert set(gold["D_each"]) == {"chi2", "lambda", "tempChi", "currentChi"} and all(v < 1e-6 for v in gold["D_each"].values())
    by = {r["name"]: r["base"] for r in rows}
    assert all(b["rounds"] == 1 and b["trial_log"]["accepted"].sum() >= 5 for b in by.values())
    assert by["e130_robust"]["not_included"][-2:].all()


def test_the_520_golden_was_made_from_the_scene():
    gold, sha, d, each = ES.load_520()
    _, g, opt = ES.scene("e520")
    assert sha == LS.input_hash(g) and g["nfree"] == 520
    assert gold["poses_d"].shape == (520, 7) and gold["points_d"].shape == (len(g["points"]), 3) and len(gold["chi2"]) == len(g["e_point"])
    log = gold["trial_log"]
    assert gold["rounds"] == 1 and log["accepted"].all() and (np.abs(log["rho"]) > 0.5).all() and sum(gold["trials"]) == len(log) >= 5
    assert 0 < d < 1e-9 and set(each) == {"chi2", "lambda", "tempChi", "currentChi"} and all(v < 1e-6 for v in each.values())
    assert os.path.getsize(ES.GOLDEN_520) < 400 * 1024


# ------------------------------------------------------------------------------------------------ 4. the sources
def test_one_body_in_the_ba_unit():
    ba = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_ba.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*(?:\{\})?;", ba, re.M)) == 1 and "WorkspaceLease" not in ba
    assert ba.count("orbm_llt_env_solve_dev(") == 1 and ba.count("k_ba_schur_env, dim3(") == 1 and ba.count("return ba_run(") == 3
    assert "hipMemsetAsync(D.A, 0" in ba                                           # the zeroing pass in front of the Schur pass
    case = open(os.path.join(ROOT, "tests", "test_gpu_ba_env_workspace.py")).read()
    assert "W.FILLS" in case and "fill_workspaces" in case and "bundle.run_global_env" in case and "e70_drop" in case


def test_shell_sorts_by_mnid_calls_the_new_entry_once_and_refuses_before_any_write():
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, header_text = _declarations()
    raw = open(os.path.join(ROOT, "integration", "Optimizer_ba_env_hip.cc")).read()
    src = _strip_comments(raw)
    calls = [(fn, n) for fn, n in _calls(raw) if fn in decl]
    assert calls == [("orbm_global_bundle_adjustment_env", 5), ("orbx_last_error", 0)]
    assert decl["orbm_global_bundle_adjustment_env"] == 5 and hasattr(_lib.lib(), "orbm_global_bundle_adjustment_env")
    body = src[src.index("bool HipBundleAdjustmentEnv"):]
    assert re.search(r"bool HipBundleAdjustmentEnv\(const std::vector<KeyFrame \*> &vpKFs, const std::vector<MapPoint \*> &vpMP, int nIterations,\s*"
                     r"bool \*pbStopFlag,\s*const unsigned long nLoopKF, const bool bRobust\)", body)
    sort, number, call = body.index("std::sort("), body.index("kfIndex["), body.index("orbm_global_bundle_adjustment_env(")
    assert "mnId < b->mnId" in body[sort:number] and sort < number < call           # sorted by mnId before the keyframes are numbered
    falses = [m.start() for m in re.finditer(r"return false;", body)]
    writes = [m.start() for m in re.finditer(r"->\w+\s*=[^=]|SetPose|SetWorldPos|copyTo|\.create\(", body)]
    assert len(falses) >= 3 and writes and max(falses) < min(writes)               # every refusal comes before anything is written
    assert "> 4096) return false;" in body[:call] and "ORBX_ERR_UNSUPPORTED) return false;" in body
    for f, _ in bundle.BaGraph._fields_:
        assert f"g.{f} =" in src, f
    for f, _ in bundle.BaResult._fields_:
        assert src.count(f"res.{f} = ") == 1, f
    assert "ORBM_BA_OPTIONS_GLOBAL(nIterations, bRobust)" in src and "mTcwGBA" in src and "mPosGBA" in src and "UpdateNormalAndDepth" in src
    for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", src)):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    old = open(os.path.join(ROOT, "integration", "Optimizer_ba_hip.cc")).read()
    assert "orbm_global_bundle_adjustment_env" not in old and "HipBundleAdjustmentEnv" not in old
    for doc in ("integration/README.md", "INTEGRATION.md"):
        assert "Optimizer_ba_env_hip.cc" in open(os.path.join(ROOT, doc)).read(), doc
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    assert re.search(r"bool GlobalMapEnv\(int nIterations, bool bRobust, const volatile uint8_t \*pbStopFlag = nullptr, orbm_ba_stats \*stats = nullptr\)", hpp)
    assert "LIST THEM BY ASCENDING mnId" in open(os.path.join(ROOT, "include", "orbslam_hip.h")).read()
