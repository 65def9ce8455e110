"""orbm_global_bundle_adjustment_env on the MI355X: up to 4,096 free keyframes, the reduced system in the live tiles of
its tile envelope, always through orbm_llt_env_solve_dev.
  The contract, device against device: every scene both entries accept -- the 16 of tests/ba_scenes.py, the 6 of
  tests/ba_large_scenes.py (full envelopes) and the banded ones of tests/ba_env_scenes.py up to e130 with e70_drop -- gives, through
  run_global_env, every output of run_global (orbm_global_bundle_adjustment) as the SAME NUMBERS (np.array_equal), with NO tolerance:
  the entries of S are the same operations in the same order and the solver skips only products with exact zeros.
  Past 512 keyframes: e520 against the golden tests/golden/ba_env_520.npz and e65_shuffled against the restatement on the shuffled
  graph -- every integer equal, the continuous outputs within M = 8 times the largest of the restatement's measured sensitivities
  (D_cpu, D_large, D_env: measured on the restatement alone, never on the device).
  e1024 and e4096 have no restatement (it would take minutes): the same bytes twice, waits, the solver's launches against the plan,
  the fixed keyframe, descent and the stored chi2 against tests/ba_optimum.py's float64 numpy model, and a noise-free e1024 that
  returns to its planted configuration.
  Limits, the stop flag, the C++ class.  The stale-arena case is tests/test_gpu_ba_env_workspace.py."""
import ctypes as C
import json
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import ba_compare
import ba_env_scenes as ES
import ba_large_scenes as LS
import ba_optimum
import ba_oracle
import ba_scenes
from orb_slam2_e_amd import _lib, bundle
from test_gpu_ba_large import KEYS, _continuous_within_the_margin, _integers_equal, image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSUPPORTED = -5
_SMALL, _LARGE, _ENV = json.load(open(ba_compare.GOLDEN)), json.load(open(LS.GOLDEN)), json.load(open(ES.GOLDEN))
INTS = ("iterations", "trials", "results", "stopped", "rounds", "ntrials", "trial_overflow", "waits")


@pytest.fixture(scope="module", autouse=True)
def margins():
    """test_gpu_ba_large's comparison with D_env among the sensitivities: D = max(D_cpu, D_large, D_env), D_each likewise"""
    import test_gpu_ba_large as TL
    old = TL.D, TL.D_EACH
    TL.D = max(_SMALL["D_cpu"], _LARGE["D_cpu"], _ENV["D_env"])
    TL.D_EACH = {k: max(_SMALL["D_each"][k], _LARGE["D_each"][k], _ENV["D_each"][k]) for k in _SMALL["D_each"]}
    yield
    TL.D, TL.D_EACH = old


def _same_numbers(new, old, name):
    """every output of two calls with statistics: np.array_equal on every array (no tolerance; == holds across the sign of a zero,
    which is all the two solvers may differ in), the trial log field by field, the integers"""
    for k in KEYS:
        if k == "trial_log":
            assert len(new[k]) == len(old[k]), name
            for f in new[k].dtype.names:
                assert np.array_equal(new[k][f], old[k][f]), (name, "trial_log", f)
        else:
            assert np.array_equal(new[k], old[k]), (name, k)
    for k in INTS:
        assert new[k] == old[k], (name, k)


def _all_scenes():
    return ba_scenes.scenes() + LS.scenes([s[0] for s in LS.SPECS]) + ES.scenes(ES.EQUAL)


def test_the_same_graph_through_both_global_entries_gives_the_same_numbers():
    names = []
    for name, g, opt in _all_scenes():
        old, new = bundle.run_global(g, opt, want_stats=True), bundle.run_global_env(g, opt, want_stats=True)
        _same_numbers(new, old, name)
        names.append(name)
    assert len(names) == 16 + 6 + 5
    # e70_drop: the keyframe in the middle left the second round's system (its rows were planned again from the read-back)
    d = bundle.run_global_env(*ES.scene("e70_drop")[1:], want_stats=True)
    assert d["rounds"] == 2 and d["level"][ES.scene("e70_drop")[1]["e_cam"] == 35].all() and d["trials"][1] > 0


@pytest.fixture(scope="module")
def device_520():
    _, g, opt = ES.scene("e520")
    return bundle.run_global_env(g, opt, want_stats=True)


def test_520_keyframes_against_the_golden(device_520):
    gold, sha, d520, each520 = ES.load_520()
    _, g, _ = ES.scene("e520")
    import test_gpu_ba_large as TL
    TL.D = max(TL.D, d520)                                                          # its own sensitivity (4 ulp patterns) joins the others
    TL.D_EACH = {k: max(v, each520[k]) for k, v in TL.D_EACH.items()}
    assert sha == LS.input_hash(g)
    with pytest.raises(_lib.OrbxError) as e:                                        # one past the dense entry's limit
        bundle.run_global(g, bundle.global_options(10, False))
    assert e.value.code == ERR_UNSUPPORTED
    _integers_equal(device_520, gold, "e520")
    _continuous_within_the_margin([("e520", device_520, gold)])
    assert device_520["waits"] == sum(device_520["trials"]) + device_520["rounds"]
    assert _lib.lib().orbm_debug_last_llt_launches() == bundle.plan_global_env(g)["launches"]


def test_shuffled_keyframes_against_the_restatement_on_the_shuffled_graph():
    _, g, opt = ES.scene("e65_shuffled")
    band, wide = bundle.plan_global_env(ES.scene("e65_loop")[1]), bundle.plan_global_env(g)
    assert wide["live_tiles"] > band["live_tiles"]
    d, r = bundle.run_global_env(g, opt, want_stats=True), ba_oracle.run(g, opt)
    _integers_equal(d, r, "e65_shuffled")
    _continuous_within_the_margin([("e65_shuffled", d, r)])


# ------------------------------------------------------------------------------------------------ sizes without a restatement
@pytest.fixture(scope="module")
def device_1024():
    _, g, opt = ES.scene("e1024")
    r = bundle.run_global_env(g, opt, want_stats=True)
    return r, _lib.lib().orbm_debug_last_llt_launches()


@pytest.fixture(scope="module")
def device_4096():
    _, g, opt = ES.scene("e4096")
    r = bundle.run_global_env(g, opt, want_stats=True)
    return r, _lib.lib().orbm_debug_last_llt_launches()


def _consistent(name, d, launches):
    """waits, launches, the fixed keyframe, descent and the stored chi2 against the numpy model.  The bound on the stored chi2 is
    ba_optimum's: the model divides in double where the code under test keeps the reference's float invz, which moves a stereo edge's
    chi2 by 1e-4 relative; 1e-3 is allowed, on the scale max(chi2, 1) of ba_compare.rel_each (1 is the scale of an ordinary edge)."""
    _, g, opt = ES.scene(name)
    assert d["waits"] == sum(d["trials"]) + d["rounds"] and d["rounds"] == 1 and d["stopped"] == 0, name
    assert d["iterations"][0] == opt.iterations[0] and d["trial_log"]["ok2"].all(), name
    assert launches == bundle.plan_global_env(g)["launches"], name
    # keyframe 0 is fixed: what comes back is toCvMat(toSE3Quat(input)), a float matrix through a double unit quaternion and back, which
    # may round an entry of magnitude <= 1 by a few float ulps (1.2e-7 each): 1e-6 is allowed
    assert g["fixed"][0] == 1 and np.abs(d["poses"][0] - g["poses"][0]).max() <= 1e-6, name
    start, _ = ba_optimum.edge_chi2(g, _input_estimates(g), g["points"].astype(np.float64))
    end, depth = ba_optimum.edge_chi2(g, d["poses_d"], d["points_d"])
    print(name, "chi2 at the input %.6e" % start.sum(), "at the result %.6e" % end.sum(), "trials", d["trials"],
          "largest |stored - recomputed| / max(chi2, 1): %.3e" % ba_compare.rel_each(d["chi2"], end, 1.0))
    assert end.sum() < start.sum() and (depth > 0).all(), name
    assert d["trial_log"]["accepted"][-1] == 1, name                               # so the stored error is the one at the returned estimates
    assert ba_compare.rel_each(d["chi2"], end, 1.0) <= 1e-3, name


def _input_estimates(g):
    """(q, t) of the free keyframes' input poses: what the call starts from (only the rotation matrix is used by the model)"""
    P = g["poses"][:g["nfree"]].reshape(-1, 4, 4).astype(np.float64)
    out = np.zeros((g["nfree"], 7))
    for k, T in enumerate(P):
        R = T[:3, :3]
        w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2                # the scenes' rotations are small: w is near 1
        out[k, :4] = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
        out[k, 4:] = T[:3, 3]
    return out


def test_1024_keyframes_are_consistent(device_1024):
    _consistent("e1024", *device_1024)


def test_1024_keyframes_twice_give_the_same_bytes(device_1024):
    _, g, opt = ES.scene("e1024")
    assert image(bundle.run_global_env(g, opt, want_stats=True)) == image(device_1024[0])


def test_4096_keyframes_are_accepted_and_consistent(device_4096):
    _, g, _ = ES.scene("e4096")
    assert g["nfree"] == 4096
    _consistent("e4096", *device_4096)


def _planted_error(g, r):
    """largest distance of a returned point from its planted position, in metres"""
    connected = r["not_included"] == 0
    return float(np.linalg.norm(r["points_d"][connected] - g["truth"][connected], axis=1).max())


def test_a_noise_free_1024_keyframe_map_returns_to_its_planted_configuration():
    """Without pixel noise the planted poses and points are a minimum with chi2 = 0 up to the floats the observations are held in, and
    keyframe 0, fixed, with the stereo edges pins the gauge.  Started off it (the scenes' start errors), the call must come back.
    The measure: the largest distance of a returned point from its planted position.  The bound: 10 times what the RESTATEMENT
    reaches on the noise-free e130_robust by the same measure with the same options, computed here; both numbers are printed
    (DESIGN.md 29 records them).  The options are optimize(64), the library's largest: a chain of keyframes anchored at one end
    has weak bending modes that Levenberg's damping holds back until lambda has shrunk, so after optimize(10) the far end is still
    1e-4 m off at 130 keyframes and 1.4e-3 m at 260 and 520 IN THE RESTATEMENT (chi2 already below 1e-5): ten iterations measure the
    length of the chain, not the code.  Run until g2o's own stop rule ends it, the restatement reaches 1.7e-5 m at 130 and 1.6e-5 m
    at 260 keyframes: the floor of the float observations, independent of the length."""
    opt = bundle.global_options(64, False)
    _, g130, _ = ES.scene("e130_robust", noise_px=0.0)
    ref = _planted_error(g130, ba_oracle.run(g130, opt))
    _, g, _ = ES.scene("e1024", noise_px=0.0)
    start = float(np.linalg.norm(g["points"] - g["truth"], axis=1).max())
    d = bundle.run_global_env(g, opt, want_stats=True)
    got = _planted_error(g, d)
    print("noise-free, optimize(64): restatement on e130 %.3e m, device on e1024 %.3e m (start %.3e m), bound %.3e m; iterations %s trials %s" %
          (ref, got, start, 10 * ref, d["iterations"], d["trials"]))
    assert got <= 10 * ref and got < start / 10


# ------------------------------------------------------------------------------------------------ limits, stop flag, C++
def _call_env(g, opt, sizes=None):
    """orbm_global_bundle_adjustment_env with sentinel-filled outputs; returns (rc, outputs untouched)"""
    L = _lib.lib()
    cg = bundle.c_graph(g)
    for k, v in (sizes or {}).items():
        setattr(cg, k, v)
    nfree, npts, ne = g["nfree"], len(g["points"]), len(g["e_point"])
    poses = np.full((nfree + 8, 16), 7.5, np.float32); points = np.full((npts + 1, 3), 7.5, np.float32)
    erase = np.full(ne + 1, 77, np.uint8); notinc = np.full(npts + 1, 77, np.uint8)
    res = bundle.BaResult(bundle.ptr(poses), bundle.ptr(points), bundle.ptr(erase), bundle.ptr(notinc), 77)
    rc = L.orbm_global_bundle_adjustment_env(C.byref(cg), C.byref(opt), None, C.byref(res), None)
    untouched = (poses == 7.5).all() and (points == 7.5).all() and (erase == 77).all() and (notinc == 77).all() and res.stopped == 77
    return rc, bool(untouched)


def test_every_cap_is_refused_with_the_outputs_untouched(device_4096):
    assert device_4096[0]["iterations"][0] == 3                                     # 4,096 keyframes ran (above)
    _, g, opt = ES.scene("e65_loop")
    done = bundle.run_global_env(g, opt)["waits"]
    assert done > 0
    for sizes in ({"nfree": 4097}, {"nfixed": 1025}, {"npoints": (1 << 20) + 1}, {"nedges": (1 << 22) + 1}):
        assert _call_env(g, opt, sizes) == (ERR_UNSUPPORTED, True), sizes
    wide = ES.wide_graph()                                                          # the tile cap: tests/test_cpu_ba_env.py plans it
    assert _call_env(wide, bundle.global_options(10, False)) == (ERR_UNSUPPORTED, True)
    assert b"8,192" in _lib.lib().orbx_last_error()
    assert _lib.lib().orbm_debug_last_ba_waits() == done                            # a refused call does not get as far as the counter


def test_stop_flag_set_before_the_call_changes_nothing_and_launches_nothing():
    _, g, opt = ES.scene("e65_loop")
    r = bundle.run_global_env(g, opt, stop_flag=np.ones(1, np.uint8), want_stats=True)
    assert r["stopped"] == 1 and r["waits"] == 0 and r["ntrials"] == 0
    assert np.array_equal(r["poses"], g["poses"][:g["nfree"]]) and np.array_equal(r["points"], g["points"]) and not r["erase"].any()
    assert _lib.lib().orbm_debug_last_ba_waits() == 0


def test_stop_flag_set_by_a_thread_gives_a_legal_outcome():
    """As tests/test_gpu_ba.py's: WHEN the thread's store lands is not controlled, so the result must be the restatement's for SOME
    position of the flag among g2o's reads (0 = never seen), within the margin.  e70_drop: the local form, both rounds."""
    _, g, opt = ES.scene("e70_drop")
    bundle.run_global_env(g, opt)                                                   # the arena has its size: the timed call does not allocate
    flag = np.zeros(1, np.uint8)

    def set_later():
        time.sleep(0.004)
        flag[0] = 1
    th = threading.Thread(target=set_later)
    th.start()
    d = bundle.run_global_env(g, opt, stop_flag=flag, want_stats=True)
    th.join()
    full = ba_oracle.run(g, opt)
    legal = [full] + [ba_oracle.run(g, opt, stop_at=k) for k in range(1, full["nreads"] + 1)]
    match = [r for r in legal if ba_compare.ints(r) == ba_compare.ints(d)]
    print("stopped", d["stopped"], "iterations", d["iterations"], "trials", d["trials"], "legal outcomes", len(legal), "matching", len(match))
    assert match
    import test_gpu_ba_large as TL
    assert min(max(ba_compare.diffs(d, r).values()) for r in match) <= ba_compare.M * TL.D


def test_through_the_cxx_class(tmp_path):
    """orbslam_hip::BundleAdjustment::GlobalMapEnv (include/orbslam_hip.hpp) on e65_loop gives the Python call's bytes."""
    libdir = os.path.join(ROOT, "orb_slam2_e_amd")
    exe = str(tmp_path / "ba_env_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "ba_env_smoke.cpp"), "-o", exe, "-L", libdir, "-lorbslam_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    _, g, opt = ES.scene("e65_loop")
    d = bundle.run_global_env(g, opt)
    nfree, npose, npts, ne = g["nfree"], len(g["poses"]), len(g["points"]), len(g["e_point"])
    sp, op = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(sp, "wb") as f:
        f.write(np.array([nfree, npose - nfree, npts, ne], np.int32).tobytes())
        for k in ("poses", "fixed", "points", "e_point", "e_cam", "e_obs", "e_inv_sigma2", "e_cam_k"):
            f.write(g[k].tobytes())
    out = subprocess.run([exe, sp, op], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    raw = open(op, "rb").read()
    assert raw[:4] == np.int32(d["stopped"]).tobytes()
    assert raw[4:4 + 64 * nfree] == d["poses"].tobytes()
    assert raw[4 + 64 * nfree:4 + 64 * nfree + 12 * npts] == d["points"].tobytes()
    assert raw[4 + 64 * nfree + 12 * npts:] == d["not_included"].tobytes()
