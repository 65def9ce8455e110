"""Tracking::TrackWithMotionModel / TrackLocalMap as one call each: the restatement (tests/track_reference.py) held to answers that
need no device -- the retry rule, the two counts, the union rule, "not tracked leaves the pose alone" -- and the ABI surface of
orbm_track_with_motion_model / orbm_track_local_map (declared, exported, refusing without a device, struct mirror = C layout)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_reference as tr
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd.matcher import Frame, ORBmatcher, Points, TrackResult, View
from orb_slam2_e_amd.synth import synth_tracking_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_search(counts):
    """a search that returns counts[0] matches at its first call, counts[1] at its second; records the windows it was asked for"""
    calls = []

    def search(fr, Tcw, Tlw, last, th, mono, check_orientation):
        nm = counts[len(calls)]
        calls.append(th)
        mk = np.full(40, -1, np.int32); mk[:nm] = np.arange(nm)
        mq = np.full(40, -1, np.int32); mq[:nm] = np.arange(nm)
        return mk, mq, nm
    return search, calls


def _stub_solve(outlier):
    def solve(fr, posecam, has, pos, Tcw):
        out = np.where(has > 0, np.asarray(outlier, np.uint8)[:len(has)], 0).astype(np.uint8)
        T = np.array(Tcw, np.float32).reshape(4, 4).copy(); T[0, 3] += 1.0
        return int(((has > 0) & (out == 0)).sum()), T, out, None
    return solve


LAST40 = dict(pos=np.arange(120, dtype=np.float32).reshape(40, 3), takes=(np.arange(40) % 3 != 0).astype(np.uint8))


@pytest.mark.parametrize("first,second,used,tracked", [(20, None, 1, True), (19, 20, 2, True), (19, 19, 2, False), (0, 40, 2, True)])
def test_retry_rule_at_19_and_20(first, second, used, tracked):
    search, calls = _stub_search([first, second])
    T = np.eye(4, dtype=np.float32)
    r = tr.track_with_motion_model(None, None, T, T, LAST40, 15.0, True, search=search, solve=_stub_solve(np.zeros(40)))
    assert calls == ([15.0] if used == 1 else [15.0, 30.0])
    assert (r["search_used"], r["tracked"]) == (used, tracked)
    assert r["nsearch"] == (first if used == 1 else second)
    if not tracked:                 # :1251-1252: no solve, the pose stays
        assert np.array_equal(r["Tcw_out"], T) and r["outlier"] is None and r["stats"] is None and r["ngood"] == 0
        assert (r["match_kp"] >= 0).sum() == second
    else:
        assert r["Tcw_out"][0, 3] == 1.0


def test_min_matches_moves_the_rule():
    search, calls = _stub_search([7, 9])
    T = np.eye(4, dtype=np.float32)
    r = tr.track_with_motion_model(None, None, T, T, LAST40, 7.0, False, min_matches=8, search=search, solve=_stub_solve(np.zeros(40)))
    assert calls == [7.0, 14.0] and r["tracked"] and r["search_used"] == 2 and r["nsearch"] == 9


def test_counts_on_hand_made_flags():
    has = np.array([1, 1, 1, 0, 1, 1, 0, 1], np.uint8)
    out = np.array([0, 1, 0, 1, 0, 1, 0, 0], np.uint8)        # (flags on empty slots do not count)
    takes = np.array([1, 1, 0, 1, 1, 0, 1, 1], np.uint8)
    assert tr.counts(has, out, takes) == (4, 3)
    assert tr.counts(np.zeros(8), out, takes) == (0, 0)
    search, _ = _stub_search([30, None])
    outl = np.zeros(40, np.uint8); outl[[0, 1, 2, 35]] = 1        # 35 holds no point
    T = np.eye(4, dtype=np.float32)
    r = tr.track_with_motion_model(None, None, T, T, LAST40, 15.0, True, search=search, solve=_stub_solve(outl))
    # 30 matches, 3 outliers; takes = index % 3 != 0: of 3 .. 29, nine are multiples of 3
    assert (r["nmatches"], r["nmatches_map"], r["ngood"]) == (27, 18, 27)
    assert np.array_equal(r["match_kp"][:3], [0, 1, 2])          # the discard does not edit the search's arrays


def test_union_rule():
    mk = np.array([4, -1, -1, 2, -2, -1], np.int32)
    ppos = np.arange(15, dtype=np.float32).reshape(5, 3); ptk = np.array([1, 1, 0, 1, 1], np.uint8)
    bh = np.array([1, 1, 0, 0, 1, 0], np.uint8); bpos = -np.ones((6, 3), np.float32); bt = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    has, pos, takes = tr.union(mk, ppos, ptk, bh, bpos, bt)
    assert list(has) == [1, 1, 0, 1, 1, 0]
    assert np.array_equal(pos[0], ppos[4]) and takes[0] == 1         # a match over an unobserved base point replaces it
    assert np.array_equal(pos[1], bpos[1]) and takes[1] == 1         # base kept
    assert np.array_equal(pos[3], ppos[2]) and takes[3] == 0         # a new match on an empty slot
    assert np.array_equal(pos[4], bpos[4]) and takes[4] == 0         # -2 is no match: the base entry stays


def test_an_observed_base_point_blocks_its_slot_an_unobserved_one_is_replaced():
    s = synth_tracking_scene(31, n=400, nmp=500)
    rng = np.random.default_rng(2)
    npnt = len(s["pos"])
    pts = dict(valid=np.ones(npnt, np.uint8), pos=s["pos"], normal=s["normal"], mind=s["mind"], maxd=s["maxd"], desc=s["mp_desc"],
               takes=np.ones(npnt, np.uint8))
    n = len(s["kps"])
    free = tr.search_points(s, s["Tcw"], pts, np.zeros(n, np.uint8), 3.0, 0.8)[0]
    hit = np.nonzero(free >= 0)[0]
    assert len(hit) > 40
    bh = np.zeros(n, np.uint8); bt = np.zeros(n, np.uint8)
    bh[hit[:20]] = 1; bt[hit[:10]] = 1                               # ten observed, ten unobserved base points under would-be matches
    bpos = rng.normal(size=(n, 3)).astype(np.float32)
    calls = []

    def solve(fr, posecam, has, pos, Tcw):
        calls.append((has.copy(), pos.copy()))
        return 0, np.array(Tcw, np.float32).reshape(4, 4), np.zeros(len(has), np.uint8), None
    r = tr.track_local_map(s, None, s["Tcw"], pts, bh, bpos, bt, 3.0, 0.8, solve=solve)
    has, pos = calls[0]
    assert (r["match_kp"][hit[:10]] < 0).all() and np.array_equal(pos[hit[:10]], bpos[hit[:10]])
    rep = hit[10:20][r["match_kp"][hit[10:20]] >= 0]
    assert len(rep) > 0 and np.array_equal(pos[rep], s["pos"][r["match_kp"][rep]])
    assert has[hit[:20]].all() and r["nmatches"] == int(has.sum()) and r["nmatches_map"] == r["nmatches"] - (10 - len(rep))


# ------------------------------------------------------------------------------------------------------- the ABI surface

NEW = ("orbm_track_with_motion_model", "orbm_track_local_map", "orbm_debug_last_track_waits")


def test_symbols_are_declared_and_exported():
    so = _lib.build()
    protos = _lib.prototypes()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = set(re.findall(r"^\S+ \S (orbm_\w+)$", out, re.M))
    for name in NEW:
        assert name in protos and name in exported, name
    vp = C.c_void_p
    assert protos["orbm_track_with_motion_model"] == (C.c_int, [vp] * 6 + [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 6)
    assert protos["orbm_track_local_map"] == (C.c_int, [vp] * 8 + [C.c_float, C.c_float, C.c_int, C.c_float] + [vp] * 7)
    assert _lib.lib().orbx_abi_version() == 136


def test_track_result_mirror_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "track_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "track_layout.c"), "-o", exe])
    lines = [l.split() for l in subprocess.check_output([exe]).decode().splitlines()]
    assert lines[0] == ["struct", "orbm_track_result", str(C.sizeof(TrackResult))]
    fields = [(l[2], int(l[3]), int(l[4])) for l in lines[1:]]
    assert fields == [(f[0], getattr(TrackResult, f[0]).offset, getattr(TrackResult, f[0]).size) for f in TrackResult._fields_]


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_device(), reason="a device is present: the calls run (tests/test_gpu_track.py)")
def test_both_calls_refuse_without_a_device():
    L = _lib.lib()
    T = np.eye(4, dtype=np.float32).reshape(16)
    sc = np.ones(8, np.float32)
    view = View(500.0, 500.0, 320.0, 240.0, 0.08, 40.0, 0.18, sc)
    cam = (C.c_float * 5)()                    # stands for an orbm_pose_camera / frame: the device test comes first
    res = TrackResult()
    pts = Points(np.zeros(1, np.uint8), np.zeros((1, 3), np.float32), np.zeros((1, 32), np.uint8))
    fake = C.c_void_p(C.addressof(cam))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.orbm_track_with_motion_model(fake, C.byref(view.c), fake, p(T), p(T), C.byref(pts.c), 15.0, 1, 95, 1, 20, None, None, None, p(T.copy()),
                                        C.byref(res), None)
    assert rc == -2, rc                        # ORBX_ERR_NO_DEVICE
    rc = L.orbm_track_local_map(fake, C.byref(view.c), fake, p(T), C.byref(pts.c), None, None, None, 1.0, 0.5, 95, 0.8, None, None, None, None,
                                p(T.copy()), C.byref(res), None)
    assert rc == -2, rc
    assert b"no usable HIP device" in L.orbx_last_error()


def test_integration_shell_calls_the_declared_entry_points():
    """integration/Tracking_track_hip.cc cannot be compiled here (no OpenCV); its C-ABI calls are checked against the headers as
    tests/test_cpu_integration_shells.py checks the other shells: declared, with that many arguments."""
    from test_cpu_integration_shells import _calls, _declarations, _strip_comments
    decl, header_text = _declarations()
    src = open(os.path.join(ROOT, "integration", "Tracking_track_hip.cc")).read()
    called = {}
    for fn, nargs in _calls(src):
        if fn not in decl:
            assert re.search(r"\b%s\b" % fn, header_text), fn
            continue
        assert decl[fn] == nargs, f"{fn} called with {nargs} arguments, declared with {decl[fn]}"
        called[fn] = called.get(fn, 0) + 1
    assert called.get("orbm_track_with_motion_model") == 1 and called.get("orbm_track_local_map") == 1
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", _strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    for word in ("HipTrackWithMotionModel", "HipTrackLocalMap", "SetPose", "mvbOutlier", "mbTrackInView", "mnLastFrameSeen", "IncreaseFound"):
        assert word in src, word
