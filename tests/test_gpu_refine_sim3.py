"""orbm_refine_sim3_candidates on the device (orbm_refine_sim3.hip): SearchBySim3 chained into OptimizeSim3 for up to 64 attempts
against one current keyframe, on the scenes of tests/refine_sim3_scenes.py.

* bit for bit the composition of what exists without it -- SearchBySim3Whole, the numpy walk of Optimizer.cc:1483-1520
  (tests/refine_sim3_reference.py), optimize_sim3 -- for every scene and every output: no tolerance;
* against the CPU restatement: the integers equal (every scene passes the selection rule on the restatement alone,
  tests/test_cpu_refine_sim3.py: none is left out), (q, t, s) within M = 8 times the larger of the scenes' own sensitivity
  (tests/golden/refine_sim3_sensitivity.json) and D_cpu of tests/golden/sim3_opt_sensitivity.json;
* the same bytes alone, at any place of a ragged batch, inside 64 attempts and on a second call; one host wait, none when nothing is
  launched; a fixed scale keeps its input bits; refusals leave every output untouched; the C++ wrapper's bytes; the fold."""
import json
import struct
import subprocess

import numpy as np
import pytest

import refine_sim3_reference as ref
import refine_sim3_scenes as scenes
import test_cpu_sim3_opt as cpu_opt
from orb_slam2_e_amd import Frame, ORBmatcher, Points, View
from orb_slam2_e_amd import sim3 as s3
from orb_slam2_e_amd._lib import OrbxError
from test_cpu_refine_sim3 import GOLDEN, attempts, build_smoke, restated

pytestmark = pytest.mark.gpu

ISG = scenes.INV_SIGMA2
M = cpu_opt.M
D = max(json.load(open(GOLDEN))["D_cpu"], json.load(open(cpu_opt.GOLDEN))["D_cpu"])
BATCHES = scenes.batches()
SINGLES = [n for n, (_, atts) in BATCHES.items() if len(atts) == 1]
_FRAMES, _OUT = {}, {}


def view():
    return View(*scenes.CAM, 0.08, 40.0, scenes.LOG_SF, scenes.SF)


def frame(key, kps, desc):
    if key not in _FRAMES:
        _FRAMES[key] = Frame(kps, desc, scenes.BOUNDS)
    return _FRAMES[key]


def kf1_of(fam):
    return (frame(("kf1", fam["seed"], fam["n1"], fam["fix_scale"]), fam["kps1"], fam["desc1"]),
            Points(fam["valid1"], fam["pos1"], fam["mp_desc"], min_distance=fam["mind1"], max_distance=fam["maxd1"]))


def kf2_of(a, valid=None):
    return (frame(("kf2", a["name"]), a["kps2"], a["desc2"]),
            Points(a["valid2"] if valid is None else valid, a["pos2"], a["mp_desc2"], min_distance=a["mind2"], max_distance=a["maxd2"]))


def call(atts, fixed, seeds=True, **kw):
    """the attempts of one family in one call: [(found12, nfound, matches12, result)], waits"""
    fam = atts[0]["family"]
    k1, p1 = kf1_of(fam)
    keep = [kf2_of(a) for a in atts]
    arr = [s3.RefineSim3Attempt(k2, p2, a["T2w"], a["R12"], a["t12"], a["s12"], a["seed12"] if seeds else None) for a, (k2, p2) in zip(atts, keep)]
    out = s3.refine_sim3_candidates(k1, p1, scenes.T1W, view(), ISG, arr, scenes.TH, scenes.TH_HIGH, scenes.TH2, fixed, **kw)
    return out, s3.last_refine_sim3_waits()


def as_bytes(r):
    return r[0].tobytes() + struct.pack("<i", r[1]) + r[2].tobytes() + bytes(r[3])


def alone(name):
    """every single-attempt batch as a call of its own, once"""
    if name not in _OUT:
        fixed, atts = BATCHES[name]
        out, waits = call(atts, fixed)
        _OUT[name] = (out[0], waits)
    return _OUT[name]


def by_attempt(a):
    return alone(a["name"] if a["name"] in BATCHES else {"big@free": "big"}[a["name"]])[0]


def composed(a):
    """SearchBySim3Whole -> the walk -> optimize_sim3, each a device call of its own"""
    fam = a["family"]
    if a["n2"] == 0:
        found, nf = np.full(fam["n1"], -1, np.int32), 0
    else:
        v1, v2 = ref.already_matched(a)
        k1 = kf1_of(fam)[0]
        p1 = Points(v1, fam["pos1"], fam["mp_desc"], min_distance=fam["mind1"], max_distance=fam["maxd1"])
        k2, p2 = kf2_of(a, v2)
        found, nf = ORBmatcher(0.75, True).SearchBySim3Whole(k1, k2, view(), scenes.T1W, a["T2w"], a["s12"], a["R12"], a["t12"], p1, p2, scenes.TH)[:2]
    prob, idx = ref.gather(a, found)
    (res, kept), = s3.optimize_sim3([cpu_opt._dev(prob)], ISG)
    return found, int(nf), ref.scatter(a, found, idx, kept), res


@pytest.mark.parametrize("name", SINGLES)
def test_equals_the_existing_calls_composed_bit_for_bit(name):
    a = BATCHES[name][1][0]
    got, waits = alone(name)
    want = composed(a)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1], "found12 / nfound"
    assert np.array_equal(got[2], want[2]), "matches12"
    assert bytes(got[3]) == bytes(want[3]), "the result struct"
    assert waits == (1 if a["n2"] else 0)


@pytest.mark.parametrize("name", SINGLES)
def test_agrees_with_the_restatement(name):
    a = BATCHES[name][1][0]
    got, r = alone(name)[0], restated(a["name"])
    assert np.array_equal(got[0], r["found12"]) and got[1] == r["nfound"]
    assert cpu_opt._ints(got[3]) == cpu_opt._ints(r["opt"]["res"]) and np.array_equal(got[2], r["matches12"])
    v, v0 = np.array(list(got[3].q) + list(got[3].t) + [got[3].s]), r["opt"]["res"].vec()
    if got[3].ncorrespondences == 0:
        assert np.array_equal(v, v0)
        return
    d = float(np.max(np.abs(v - v0) / np.abs(v0)))
    print(name, "relative difference of (q, t, s) %.3e (8 D = %.3e)" % (d, M * D))
    assert d <= M * D


def test_an_attempt_gives_the_same_bytes_anywhere_in_a_batch_and_on_a_second_call():
    for name in ("ragged3", "p64"):
        fixed, atts = BATCHES[name]
        first, waits = call(atts, fixed)
        second, _ = call(atts, fixed)
        assert waits == 1
        for a, x, y in zip(atts, first, second):
            assert as_bytes(x) == as_bytes(by_attempt(a)) == as_bytes(y), (name, a["name"])
    fixed, atts = BATCHES["ragged3"]
    turned, _ = call(atts[::-1], fixed)
    for a, x in zip(atts[::-1], turned):
        assert as_bytes(x) == as_bytes(by_attempt(a))


def test_waits_are_one_and_none_when_nothing_is_launched():
    assert alone("both@free")[1] == 1 and alone("none@free")[1] == 1 and alone("n2_zero")[1] == 0
    k1, p1 = kf1_of(scenes.fam())
    assert s3.refine_sim3_candidates(k1, p1, scenes.T1W, view(), ISG, []) == [] and s3.last_refine_sim3_waits() == 0
    r = alone("n2_zero")[0]                                                    # the input Sim3, nin = 0, as orbm_optimize_sim3 for n = 0
    a = BATCHES["n2_zero"][1][0]
    (want, _), = s3.optimize_sim3([cpu_opt._dev(ref.gather(a, np.full(a["family"]["n1"], -1))[0])], ISG)
    assert bytes(r[3]) == bytes(want) and r[3].nin == 0 and (r[0] == -1).all() and (r[2] == -1).all() and r[1] == 0


def test_a_fixed_scale_keeps_its_input_bits():
    for name in SINGLES:
        fixed, (a,) = BATCHES[name]
        if fixed:
            assert alone(name)[0][3].s == float(a["s12"]) == 1.0, name
    assert alone("both@free")[0][3].s != float(BATCHES["both@free"][1][0]["s12"])


def test_no_seed_array_is_all_minus_one():
    fixed, atts = BATCHES["search_only@free"]
    out, _ = call(atts, fixed, seeds=False)
    assert as_bytes(out[0]) == as_bytes(alone("search_only@free")[0])


def test_refusals_leave_the_outputs_untouched():
    a = BATCHES["both@free"][1][0]
    fam = a["family"]
    k1, p1 = kf1_of(fam)
    k2, p2 = kf2_of(a)
    good = lambda **kw: s3.RefineSim3Attempt(k2, p2, a["T2w"], a["R12"], a["t12"], a["s12"], kw.get("seed", a["seed12"]))

    def refused(code, text, kf1=k1, pts1=p1, atts=None, v=None, **kw):
        atts = [good()] if atts is None else atts
        with pytest.raises(OrbxError) as e:
            s3.refine_sim3_candidates(kf1, pts1, scenes.T1W, v or view(), ISG, atts, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert s3.last_refine_sim3_waits() == 0
        return atts

    refused(-5, "64", atts=[good()] * 65)
    short = Points(fam["valid1"][:-1], fam["pos1"][:-1], fam["mp_desc"][:-1], min_distance=fam["mind1"][:-1], max_distance=fam["maxd1"][:-1])
    refused(-1, "bad arguments", pts1=short)                                   # points.n != the handle's n
    short2 = Points(a["valid2"][:-1], a["pos2"][:-1], a["mp_desc2"][:-1], min_distance=a["mind2"][:-1], max_distance=a["maxd2"][:-1])
    refused(-1, "bad arguments", atts=[good(), s3.RefineSim3Attempt(k2, short2, a["T2w"], a["R12"], a["t12"], a["s12"], a["seed12"])])
    for bad in (a["n2"], -3):
        s = a["seed12"].copy(); s[5] = bad
        refused(-1, "seed", atts=[good(), good(seed=s)])
    assert a["kps2"]["octave"].max() == 7
    refused(-1, "octave", v=View(*scenes.CAM, 0.08, 40.0, scenes.LOG_SF, scenes.SF[:7]))     # an octave outside [0, nlevels)
    # untouched: the mirror presets every output with -9 and zeroed results; a refused call must not have written any
    L = s3.lib()
    arr = (s3._CRefineSim3Attempt * 2)()
    found = np.full((2, fam["n1"]), -9, np.int32); matches = np.full((2, fam["n1"]), -9, np.int32)
    nf = np.full(2, -9, np.int32); res = (s3.Sim3OptResult * 2)()
    s = a["seed12"].copy(); s[5] = a["n2"]
    seeds = [a["seed12"], s]
    T2 = np.ascontiguousarray(a["T2w"], np.float32).reshape(16); T1 = np.ascontiguousarray(scenes.T1W, np.float32).reshape(16)
    for p, c in enumerate(arr):
        c.kf2, c.points2, c.T2w = k2._h.value if hasattr(k2._h, "value") else k2._h, s3.C.addressof(p2.c), T2.ctypes.data
        c.R12, c.t12, c.s12 = (s3.C.c_float * 9)(*a["R12"].ravel()), (s3.C.c_float * 3)(*a["t12"]), float(a["s12"])
        c.seed12, c.found12, c.matches12 = seeds[p].ctypes.data, found[p].ctypes.data, matches[p].ctypes.data
    v = view()
    rc = L.orbm_refine_sim3_candidates(k1._h, s3.C.byref(p1.c), T1.ctypes.data, s3.C.byref(v.c), ISG.ctypes.data, arr, 2, 7.5, 95, 10.0, 0,
                                       nf.ctypes.data, res)
    assert rc == -1 and (found == -9).all() and (matches == -9).all() and (nf == -9).all() and bytes(res) == bytes(len(bytes(res)))
    seeds[1][5] = -1
    rc = L.orbm_refine_sim3_candidates(k1._h, s3.C.byref(p1.c), T1.ctypes.data, s3.C.byref(v.c), ISG.ctypes.data, arr, 2, 7.5, 95, 10.0, 0,
                                       nf.ctypes.data, res)
    assert rc == 0 and (found != -9).all() and (nf >= 0).all()                 # and the accepted call writes them all


def test_the_fold_takes_the_first_attempt_with_twenty_inliers():
    fixed, atts = BATCHES["ragged3"]
    order = [atts[1], atts[2], atts[0]]                                        # the first is planted to fail (fewer than 10 pairs survive)
    out, _ = call(order, fixed)
    assert out[0][3].nin == 0 and out[1][3].nin >= 20 and out[2][3].nin >= 20
    assert s3.first_accepted(out) == 1
    assert s3.first_accepted(out[:1]) is None and s3.first_accepted([]) is None
    assert s3.first_accepted(out, min_inliers=10 ** 6) is None


def _write_batch(path, atts, fixed):
    fam = atts[0]["family"]
    f32, i32 = (lambda x: np.ascontiguousarray(x, np.float32).tobytes()), (lambda *x: struct.pack("<%di" % len(x), *x))
    with open(path, "wb") as f:
        f.write(i32(len(atts), fam["n1"], scenes.NLEVELS, int(fixed)) + f32(scenes.CAM) + f32([scenes.LOG_SF, scenes.TH, scenes.TH2]))
        f.write(f32(scenes.SF) + f32(ISG))
        f.write(fam["kps1"].tobytes() + fam["desc1"].tobytes() + fam["valid1"].tobytes() + f32(fam["pos1"]) + f32(fam["mind1"]) + f32(fam["maxd1"]))
        f.write(fam["mp_desc"].tobytes() + f32(scenes.T1W))
        for a in atts:
            f.write(i32(a["n2"]) + a["kps2"].tobytes() + a["desc2"].tobytes() + a["valid2"].tobytes() + f32(a["pos2"]) + f32(a["mind2"]))
            f.write(f32(a["maxd2"]) + a["mp_desc2"].tobytes() + f32(a["T2w"]) + f32(a["R12"]) + f32(a["t12"]) + f32([a["s12"]]))
            f.write(np.ascontiguousarray(a["seed12"], np.int32).tobytes())


def test_cxx_wrapper_gives_the_python_calls_bytes(tmp_path):
    fixed, atts = BATCHES["ragged3"]
    order = [atts[1], atts[2], atts[0]]
    src, dst = str(tmp_path / "batch.bin"), str(tmp_path / "out.bin")
    _write_batch(src, order, fixed)
    out = subprocess.run([build_smoke(tmp_path), src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK 3 attempts, accepted 1"), out.stdout + out.stderr
    want = b"".join(as_bytes(by_attempt(a)) for a in order) + struct.pack("<i", 1)
    assert open(dst, "rb").read() == want
