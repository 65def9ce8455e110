"""orbm_global_bundle_adjustment on the MI355X: up to 512 free keyframes, the reduced system always through the tiled
multi-workgroup Cholesky.
  The contract: every scene of tests/ba_scenes.py through run_global gives the BYTES of run (orbm_bundle_adjustment, one-workgroup
  solve) -- nfree64 with its 384-wide system included.
  Beyond 64 keyframes (tests/ba_large_scenes.py): every integer output equal to the restatement tests/ba_oracle.c, the continuous
  ones within M = 8 times the larger of the restatement's two measured sensitivities (tests/golden/ba_sensitivity.json, the
  project's D_cpu, and tests/golden/ba_large_sensitivity.json on these scenes: measured on the restatement alone, never on the
  device); t512_global against the golden tests/golden/ba_large_512.npz in the same measures.
  Waits, repeatability, the stop flag, stale arenas, the C++ class."""
import json
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import ba_large_scenes as LS
import ba_oracle
import ba_scenes
import workspace_cases as W
from orb_slam2_e_amd import _lib, bundle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SMALL, _LARGE = json.load(open(ba_compare.GOLDEN)), json.load(open(LS.GOLDEN))
M = ba_compare.M
D = max(_SMALL["D_cpu"], _LARGE["D_cpu"])
D_EACH = {k: max(_SMALL["D_each"][k], _LARGE["D_each"][k]) for k in _SMALL["D_each"]}
KEYS = ("poses", "points", "erase", "not_included", "poses_d", "points_d", "chi2", "level", "trial_log")


def image(r):
    """every output of a call with statistics, as bytes and integers"""
    return [r[k].tobytes() for k in KEYS] + [repr((r["iterations"], r["trials"], r["results"], r["stopped"], r["rounds"], r["ntrials"]))]


@pytest.fixture(scope="module")
def device():
    """name -> the device's result on the scenes up to t200, computed once"""
    return {name: bundle.run_global(g, opt, want_stats=True) for name, g, opt in LS.scenes(LS.MEASURED)}


@pytest.fixture(scope="module")
def reference():
    """name -> the restatement's result: computed once, shared, never changed"""
    return {name: ba_oracle.run(g, opt) for name, g, opt in LS.scenes(LS.MEASURED)}


@pytest.fixture(scope="module")
def device_512():
    _, g, opt = LS.scene("t512_global")
    return bundle.run_global(g, opt, want_stats=True)


def test_the_same_graph_through_both_entries_gives_the_same_bytes():
    names = []
    for name, g, opt in ba_scenes.scenes():
        old, new = bundle.run(g, opt, want_stats=True), bundle.run_global(g, opt, want_stats=True)
        for k, (a, b) in enumerate(zip(image(new), image(old))):
            assert a == b, f"{name}: output {k} of orbm_global_bundle_adjustment differs from orbm_bundle_adjustment's"
        assert new["waits"] == old["waits"], name
        names.append(name)
    assert len(names) == 16 and "nfree64" in names


def _integers_equal(d, r, name):
    assert np.array_equal(d["level"], r["level"]), name
    assert np.array_equal(d["erase"], r["erase"]), name
    assert np.array_equal(d["not_included"], r["not_included"]), name
    assert (d["iterations"], d["trials"], d["results"], d["stopped"], d["rounds"]) == \
           (list(r["iterations"]), list(r["trials"]), list(r["results"]), r["stopped"], r["rounds"]), name
    assert d["ntrials"] == r["ntrials"] and not d["trial_overflow"], name
    assert [tuple(t) for t in d["trial_log"][["round", "qmax", "accepted", "ok2"]]] == \
           [tuple(t) for t in r["trial_log"][["round", "qmax", "accepted", "ok2"]]], name


def _continuous_within_the_margin(pairs):
    worst, worst_each = {}, {}
    for name, d, r in pairs:
        for k, v in ba_compare.diffs(d, r).items():
            if v >= worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, name)
        for k, v in ba_compare.diffs_each(d, r).items():
            if v >= worst_each.get(k, (0.0, ""))[0]:
                worst_each[k] = (v, name)
        assert np.abs(d["points"] - d["points_d"]).max() <= 1e-6 * np.abs(d["points_d"]).max(), name
    print("largest relative differences to the restatement:", {k: "%.3e (%s)" % v for k, v in worst.items()}, "M D = %.3e" % (M * D))
    print("largest entry-by-entry differences:", {k: "%.3e (%s)" % v for k, v in worst_each.items()},
          "M D_each =", {k: "%.3e" % (M * v) for k, v in D_EACH.items()})
    for k, (v, name) in worst.items():
        assert v <= M * D, (k, name, v, M * D)
    for k, (v, name) in worst_each.items():
        assert v <= M * D_EACH[k], (k, name, v, M * D_EACH[k])


def test_every_integer_output_equals_the_restatement(device, reference):
    assert _LARGE["scenes"] == list(device) == LS.MEASURED
    for name, d in device.items():
        _integers_equal(d, reference[name], name)
    assert device["t65_local"]["rounds"] == 2 and device["t70_drop"]["level"][LS.scene("t70_drop")[1]["e_cam"] == 69].all()
    assert device["t96_global"]["not_included"][-2:].tolist() == [1, 1]


def test_continuous_outputs_agree_within_eight_times_the_sensitivity(device, reference):
    _continuous_within_the_margin([(name, d, reference[name]) for name, d in device.items()])


def test_512_keyframes_against_the_golden(device_512):
    gold, sha = LS.load_512()
    assert sha == LS.input_hash(LS.scene("t512_global")[1])
    _integers_equal(dict(device_512, trial_overflow=device_512["trial_overflow"]), gold, "t512_global")
    _continuous_within_the_margin([("t512_global", device_512, gold)])
    assert device_512["waits"] == sum(device_512["trials"]) + device_512["rounds"]


def test_host_waits_are_trials_plus_rounds(device):
    for name, d in device.items():
        assert d["rounds"] == (2 if name in ("t65_local", "t70_drop") else 1), name
        assert d["waits"] == sum(d["trials"]) + d["rounds"], name


def test_the_same_call_twice_gives_the_same_bytes(device):
    for name in ("t65_local", "t130_global_robust"):
        _, g, opt = LS.scene(name)
        assert image(bundle.run_global(g, opt, want_stats=True)) == image(device[name]), name


def test_stop_flag_set_before_the_call_changes_nothing_and_launches_nothing():
    _, g, opt = LS.scene("t96_global")
    r = bundle.run_global(g, opt, stop_flag=np.ones(1, np.uint8), want_stats=True)
    assert r["stopped"] == 1 and r["waits"] == 0 and r["ntrials"] == 0
    assert np.array_equal(r["poses"], g["poses"][:g["nfree"]]) and np.array_equal(r["points"], g["points"]) and not r["erase"].any()
    assert _lib.lib().orbm_debug_last_ba_waits() == 0


@pytest.mark.parametrize("fill", W.FILLS, ids=[f[0] for f in W.FILLS])
def test_stale_arena_contents_change_nothing(fill, device):
    _, g, opt = LS.scene("t65_local")
    _, word, as_next = fill
    nw, _ = W.fill_workspaces(word, as_next)
    assert nw >= 1
    r = bundle.run_global(g, opt, want_stats=True)
    for k, (a, b) in enumerate(zip(image(r), image(device["t65_local"]))):
        assert a == b, f"t65_local after the fill {fill[0]}: output {k} differs from the baseline"
    assert r["waits"] == device["t65_local"]["waits"]


def test_through_the_cxx_class(device, tmp_path):
    """orbslam_hip::BundleAdjustment::GlobalMap (include/orbslam_hip.hpp) on t96_global gives the Python call's bytes."""
    libdir = os.path.join(ROOT, "orb_slam2_e_amd")
    exe = str(tmp_path / "ba_global_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "ba_global_smoke.cpp"), "-o", exe, "-L", libdir, "-lorbslam_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    _, g, _ = LS.scene("t96_global")
    nfree, npose, npts, ne = g["nfree"], len(g["poses"]), len(g["points"]), len(g["e_point"])
    sp, op = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(sp, "wb") as f:
        f.write(np.array([nfree, npose - nfree, npts, ne], np.int32).tobytes())
        for k in ("poses", "fixed", "points", "e_point", "e_cam", "e_obs", "e_inv_sigma2", "e_cam_k"):
            f.write(g[k].tobytes())
    out = subprocess.run([exe, sp, op], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    raw = open(op, "rb").read()
    d = device["t96_global"]
    assert raw[:4] == np.int32(d["stopped"]).tobytes()
    assert raw[4:4 + 64 * nfree] == d["poses"].tobytes()
    assert raw[4 + 64 * nfree:4 + 64 * nfree + 12 * npts] == d["points"].tobytes()
    assert raw[4 + 64 * nfree + 12 * npts:] == d["not_included"].tobytes()
