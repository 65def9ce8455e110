"""Fuse against every target keyframe in one call (orbm_fuse_keyframes, ORBmatcher.fuse_keyframes), the part that needs no device:
the symbols are declared, exported and bound; orbm_fuse_target's C layout is the Python mirror's; the refusals that are decided
before a device is needed; the host logic of the whole loop -- mask, replay target by target, refresh of the rows of later targets
for heirs whose descriptor changed -- with the oracle standing in for the device, against the literal sequential loop of
tests/fuse_keyframes_reference.py; the C++ header's FuseKeyFrames / FuseKeyFramesSim3 against the same op log; and the integration
shell calls what the headers declare."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_keyframes_reference as R
import fuse_keyframes_scenes as S
from orb_slam2_e_amd import ORBmatcher
from orb_slam2_e_amd._lib import lib, prototypes
from orb_slam2_e_amd.matcher import _CCamera, _CFuseTarget
from test_cpu_integration_shells import _calls, _declarations, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -2, -5


def test_new_symbols_are_declared_exported_and_bound():
    protos = prototypes()
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    assert protos["orbm_fuse_keyframes"] == (i, [vp, i, i, vp, vp, vp, vp, vp, i, vp, f, f, vp, vp, i, vp, vp, vp])
    assert protos["orbm_debug_last_fuse_keyframes_waits"] == (i, [])
    L = lib()
    for name in ("orbm_fuse_keyframes", "orbm_debug_last_fuse_keyframes_waits"):
        assert getattr(L, name).argtypes == protos[name][1]
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name]).decode()
    assert " T orbm_fuse_keyframes\n" in out and " T orbm_debug_last_fuse_keyframes_waits\n" in out
    assert callable(ORBmatcher.fuse_keyframes) and callable(ORBmatcher.fuse_keyframes_rows)
    assert ORBmatcher.last_fuse_keyframes_rows_waits() >= 0 and ORBmatcher.last_fuse_keyframes_waits() >= 0
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    assert "orbm_fuse_keyframes" in hpp and "FuseKeyFramesSim3" in hpp and "struct FuseTargetView" in hpp
    assert L.orbx_abi_version() == 136          # additions only: the number stays


def test_struct_mirror_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_fuse")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_fuse.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            assert w[0] == "field"
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    for name, m, count in (("orbm_fuse_target", _CFuseTarget, 6), ("orbm_camera", _CCamera, 12)):
        assert C.sizeof(m) == sizes[name] and len(fields[name]) == count
        assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name]
    assert ORBmatcher.CAM_DTYPE.itemsize == sizes["orbm_camera"]
    assert [ORBmatcher.CAM_DTYPE.fields[n][1] for n in ORBmatcher.CAM_DTYPE.names] == [o for _, o, _ in fields["orbm_camera"]]


def _call(L, targets, K, m, nlevels=8, sim3=0, sigma=True, best=None, idx=None, arrays=True):
    f = np.zeros(max(3 * m, 3), np.float32); d = np.zeros((max(m, 1), 32), np.uint8)
    sc = np.ones(16, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return L.orbm_fuse_keyframes(targets, K, sim3, p(f) if arrays else None, p(f), p(f), p(f), p(d), m, None, 3.0, 0.18, p(sc),
                                 p(sc) if sigma else None, nlevels, p(best) if best is not None else None,
                                 p(idx) if idx is not None else None, None)


def test_refusals_that_need_no_device():
    """Sizes out of range, NULL arrays and a target without a frame are refused whatever else the call holds, before a device is
    asked for; refused calls write nothing and leave the wait counter alone.  (A non-finite pose and an octave outside the pyramid
    need a frame, which only a device can make: tests/test_gpu_fuse_keyframes.py has those.)"""
    L = lib()
    arr = (_CFuseTarget * 129)()                     # every frame NULL
    best = np.full(129 * 8, -7, np.int32); idx = np.full(129 * 8, -7, np.int32)
    before = L.orbm_debug_last_fuse_keyframes_waits()
    assert _call(L, arr, 129, 8, best=best, idx=idx) == ERR_UNSUPPORTED and b"128" in L.orbx_last_error()
    assert _call(L, arr, 1, 65537, best=best, idx=idx) == ERR_UNSUPPORTED
    assert _call(L, arr, 65, 65536, best=best, idx=idx) == ERR_UNSUPPORTED      # 65 * 65,536 > 4,194,304 pairs
    assert _call(L, arr, -1, 8, best=best, idx=idx) == ERR_ARG
    assert _call(L, arr, 1, -1, best=best, idx=idx) == ERR_ARG
    assert _call(L, None, 1, 8, best=best, idx=idx) == ERR_ARG
    assert _call(L, arr, 1, 8, best=None, idx=idx) == ERR_ARG
    assert _call(L, arr, 1, 8, best=best, idx=None) == ERR_ARG
    assert _call(L, arr, 1, 8, best=best, idx=idx, arrays=False) == ERR_ARG
    assert _call(L, arr, 1, 8, nlevels=0, best=best, idx=idx) == ERR_ARG
    assert _call(L, arr, 1, 8, nlevels=17, best=best, idx=idx) == ERR_ARG
    assert _call(L, arr, 1, 8, sigma=False, best=best, idx=idx) == ERR_ARG       # the gate is on and has no sigma
    assert _call(L, arr, 1, 8, best=best, idx=idx) == ERR_ARG                    # NULL frame
    assert _call(L, arr, 128, 8, best=best, idx=idx) == ERR_ARG                  # K = 128 is in range: it fails on its frames
    assert _call(L, arr, 1, 8, sim3=1, sigma=False, best=best, idx=idx) == ERR_ARG   # (sigma may be NULL here: the frame is what fails)
    assert (best == -7).all() and (idx == -7).all() and L.orbm_debug_last_fuse_keyframes_waits() == before


def test_without_a_device_an_empty_batch_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call(lib(), None, 0, 0) == ERR_NO_DEVICE      # (arguments first, then the device)


# ------------------------------------------------------------------------------------------------ the whole loop on the host
def oracle_stage(scene, sim3, calls):
    """the candidate stage of ORBmatcher.fuse_keyframes with the oracle standing in for the device"""
    def stage(targets, points, desc, active):
        calls.append((len(targets), len(points), int(np.count_nonzero(active))))
        return R.candidate_rows(scene, targets, points, desc, active, sim3)
    return stage


def run_whole_loop(scene, sim3, candidates):
    w = scene.world.clone()
    mt = ORBmatcher(0.8)
    n = mt.fuse_keyframes(scene.targets, scene.lst, scene.pos, scene.nrm, scene.mind, scene.maxd, scene.list_descriptors(), S.LOGSF, S.SF,
                          S.INV_SIGMA2, scene.th, R.WorldOps(scene, w, sim3), sim3=sim3, candidates=candidates)
    return n, w


def check_against_literal_loop(scene, sim3, candidates=None, calls=None):
    ref = scene.world.clone()
    n_ref, refreshes, changed = R.literal_loop(scene, ref, sim3)
    n, w = run_whole_loop(scene, sim3, candidates)
    assert n == n_ref and w.ops == ref.ops and R.same_state(w.state(), ref.state())
    assert ORBmatcher.last_fuse_keyframes_refreshes() == refreshes and ORBmatcher.last_fuse_keyframes_waits() == 1 + refreshes
    if calls is not None:
        assert len(calls) == 1 + refreshes and calls[0][:2] == (len(scene.targets), len(scene.lst))
    return n_ref, refreshes, changed, ref


def test_the_flip_needs_the_refresh():
    """Scene (a).  The literal loop fuses once per target; a replay of the first call's rows without refresh misses target 1."""
    scene = S.flip_scene()
    calls = []
    n, refreshes, changed, ref = check_against_literal_loop(scene, False, oracle_stage(scene, False, calls), calls)
    assert n == [1, 1] and refreshes == 1 and changed == 1 and calls[1][:2] == (1, 1)
    assert ref.ops == [("replace", 0, 1, 0), ("add", 1, 0, 0)] and int(ref.nobs[0]) == 5
    stale = scene.world.clone()
    n_stale, _, _ = R.literal_loop(scene, stale, False, freeze_descriptors=True)
    assert n_stale == [1, 0] and stale.ops == ref.ops[:1] and not R.same_state(stale.state(), ref.state())
    # the first call's rows: target 1's keypoint is 70 bits from the descriptor the list entry had at entry
    best, idx, vis = R.candidate_rows(scene, scene.targets, [0], scene.list_descriptors(), None, False)
    assert best[:, 0].tolist() == [40, 70] and idx[:, 0].tolist() == [0, 0] and vis[:, 0].tolist() == [1, 1]


SEEDS = {False: 11, True: 12}


@pytest.mark.parametrize("sim3", [False, True])
def test_random_scene_equals_the_literal_loop(sim3):
    """Scene (b), K = 4, m about 300; what the scene must contain is checked on the reference alone."""
    scene = S.random_scene(SEEDS[sim3], sim3=sim3)
    assert len(scene.targets) == 4 and 280 <= len(scene.lst) <= 320
    calls = []
    n, refreshes, changed, ref = check_against_literal_loop(scene, sim3, oracle_stage(scene, sim3, calls), calls)
    kinds = {op[0] for op in ref.ops}
    if sim3:
        assert kinds == {"add", "record", "caller_replace"}
    else:
        assert kinds == {"add", "replace"}
        assert any(op[0] == "replace" and op[2] < 260 for op in ref.ops) and any(op[0] == "replace" and op[2] >= 260 for op in ref.ops)
    assert min(n) > 5 and refreshes == 3 and changed == 3
    lst = scene.lst
    assert (lst < 0).sum() > 0 and len(np.unique(lst[lst >= 0])) < (lst >= 0).sum()      # NULL entries and duplicates
    heirs = [h for h in ref.heir_events if h < 260]
    assert len(heirs) > len(set(heirs))                                                    # one entry became an heir twice
    # the refreshes are small, and the result differs from a replay without them
    assert all(c[1] < len(lst) // 2 for c in calls[1:])
    stale = scene.world.clone()
    R.literal_loop(scene, stale, sim3, freeze_descriptors=True)
    assert stale.ops != ref.ops


def test_mask_is_only_an_optimisation():
    """The same loop with every pair left active (in_target answers False) gives the same result: the tails test every skip again."""
    scene = S.random_scene(SEEDS[False])
    ref = scene.world.clone()
    n_ref, refreshes, _ = R.literal_loop(scene, ref, False)

    class NoMask(R.WorldOps):
        def in_target(self, h, k): return False
    w = scene.world.clone()
    n = ORBmatcher(0.8).fuse_keyframes(scene.targets, scene.lst, scene.pos, scene.nrm, scene.mind, scene.maxd, scene.list_descriptors(),
                                       S.LOGSF, S.SF, S.INV_SIGMA2, scene.th, NoMask(scene, w), candidates=oracle_stage(scene, False, []))
    assert n == n_ref and w.ops == ref.ops and R.same_state(w.state(), ref.state())


def test_empty_lists_and_no_targets():
    scene = S.flip_scene()
    w = scene.world.clone()
    stage = lambda t, p, d, a: (np.zeros((len(t), len(p)), np.int32),) * 3
    mt = ORBmatcher(0.8)
    assert mt.fuse_keyframes([], scene.lst, scene.pos, scene.nrm, scene.mind, scene.maxd, scene.list_descriptors(), S.LOGSF, S.SF, S.INV_SIGMA2,
                             3.0, R.WorldOps(scene, w), candidates=stage) == []
    e = np.zeros((0, 3), np.float32)
    assert mt.fuse_keyframes(scene.targets, [], e, e, e[:, 0], e[:, 0], np.zeros((0, 32), np.uint8), S.LOGSF, S.SF, S.INV_SIGMA2, 3.0,
                             R.WorldOps(scene, w), candidates=stage) == [0, 0]
    assert w.ops == []


# ------------------------------------------------------------------------------------------------ the C++ header's loop
def _write_rows(f, rows):
    best, idx, vis = rows
    f.write("%d %d\n" % best.shape)
    for a in (best, idx, vis):
        f.write(" ".join(str(int(v)) for v in a.ravel()) + "\n")


@pytest.mark.parametrize("sim3", [False, True])
def test_cxx_header_loop_reproduces_the_op_log(sim3, tmp_path):
    """orbslam_hip::ORBmatcher::FuseKeyFrames / FuseKeyFramesSim3 (include/orbslam_hip.hpp) compiled with g++ over a toy map of its
    own (tests/cxx/fuse_keyframes_smoke.cpp) and a stub candidate stage that answers from a file: the rows the Python loop's stage
    returned, call by call.  The program checks that it is asked for the same points with the same descriptors and masks, and
    prints nFused, waits, refreshes and the op log."""
    scene = S.random_scene(SEEDS[sim3], sim3=sim3)
    record = []

    def stage(targets, points, desc, active):
        rows = R.candidate_rows(scene, targets, points, desc, active, sim3)
        record.append((np.array(points), np.array(desc), np.array(active), rows))
        return rows
    n, w = run_whole_loop(scene, sim3, stage)
    exe = str(tmp_path / "fuse_keyframes_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "fuse_keyframes_smoke.cpp"), "-o", exe])
    world, lst = scene.world, scene.lst
    path = str(tmp_path / "scene.txt")
    with open(path, "w") as f:
        ids = sorted(world.kfs)
        f.write("%d %d %d %d %d\n" % (int(sim3), len(world.bad), len(ids), len(scene.targets), len(lst)))
        for kfid in ids:
            kf = world.kfs[kfid]
            f.write("%d %d\n" % (kfid, len(kf.desc)))
            f.write(" ".join(str(int(v)) for v in kf.desc.ravel()) + "\n")
            f.write(" ".join(str(int(u >= 0)) for u in kf.uright) + "\n")
            f.write(" ".join(str(int(v)) for v in kf.slots) + "\n")
        for h in range(len(world.bad)):
            f.write("%d %d " % (int(world.bad[h]), len(world.obs[h])) + " ".join("%d %d" % kv for kv in sorted(world.obs[h].items())) + "\n")
            f.write(" ".join(str(int(v)) for v in world.desc[h]) + "\n")
        f.write(" ".join(str(t.id) for t in scene.targets) + "\n")
        f.write(" ".join(str(int(v)) for v in lst) + "\n")
        f.write("%d\n" % len(record))
        for points, desc, active, rows in record:
            f.write("%d %d\n" % (active.shape[0], len(points)))
            f.write(" ".join(str(int(v)) for v in points) + "\n")
            f.write(" ".join(str(int(v)) for v in desc.ravel()) + "\n")
            f.write(" ".join(str(int(v)) for v in active.ravel()) + "\n")
            _write_rows(f, rows)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip("\n").split("\n")
    assert [int(v) for v in lines[0].split()] == n
    assert [int(v) for v in lines[1].split()] == [len(record), len(record) - 1]           # waits, refreshes
    kind = {"add": 0, "replace": 1, "record": 2, "caller_replace": 3}
    assert [tuple(int(v) for v in l.split()) for l in lines[2:]] == [(kind[o[0]],) + tuple(o[1:]) for o in w.ops]
    assert len(w.ops) > 20 and len(record) == 4


def test_integration_shell_calls_the_declared_entry_point():
    """integration/LocalMapping_fuse_hip.cc cannot be compiled here (no OpenCV): its library calls have the declared numbers of
    arguments, every ORBM_ / ORBX_ constant it names exists, both hooks are defined, and the pinned patch does not carry them."""
    decl, header_text = _declarations()
    src = open(os.path.join(ROOT, "integration", "LocalMapping_fuse_hip.cc")).read()
    for fn, nargs in _calls(src):
        if fn not in decl:
            assert re.search(r"\b%s\b" % fn, header_text), f"{fn} is not in include/*.h"
            continue
        assert decl[fn] == nargs, f"{fn} called with {nargs} arguments, declared with {decl[fn]}"
        assert hasattr(lib(), fn)
    code = _strip_comments(src)
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", code)):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    assert "FuseKeyFrames(" in code and "FuseKeyFramesSim3(" in code
    assert len(re.findall(r"^bool HipFuseInTargets\(", code, re.M)) == 1
    assert len(re.findall(r"^bool HipSearchAndFuse\(", code, re.M)) == 1
    assert "LocalMapping_fuse" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
    for doc in ("INTEGRATION.md", os.path.join("integration", "README.md")):
        assert "LocalMapping_fuse_hip.cc" in open(os.path.join(ROOT, doc)).read(), doc
