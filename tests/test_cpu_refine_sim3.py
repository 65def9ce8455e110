"""orbm_refine_sim3_candidates (SearchBySim3 chained into OptimizeSim3), the part that needs no device: the restatement -- the
composition oracle.search_by_sim3_whole -> the numpy walk of Optimizer.cc:1483-1520 (tests/refine_sim3_reference.py) ->
tests/sim3_opt_oracle.py -- on the scenes of tests/refine_sim3_scenes.py: the scenes cover the shapes the call has to get right,
every one of them passes the selection rule of tests/test_cpu_sim3_opt.py on the restatement alone (0 left out), and the
sensitivity of the continuous outputs to the last bit of sin / cos / exp is the one pinned in
tests/golden/refine_sim3_sensitivity.json (tests/test_gpu_refine_sim3.py takes its tolerance from there).  Then the surfaces: ABI,
struct mirror, the refusals that need no frame handle, the C++ wrapper and the integration shell's calls."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import refine_sim3_reference as ref
import refine_sim3_scenes as scenes
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import sim3 as s3
from test_cpu_sim3_opt import CAP, M, ULP_SEEDS, _ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refine_sim3_sensitivity.json")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5


def attempts():
    """every distinct attempt of the batches, by name"""
    out = {}
    for _, atts in scenes.batches().values():
        for a in atts:
            out.setdefault(a["name"], a)
    return out


@functools.lru_cache(None)
def restated(name):
    return ref.restatement(attempts()[name])


# ------------------------------------------------------------------------------------------------ 1. the scenes
def test_scenes_cover_the_shapes():
    A = attempts()
    for fixed in ("free", "fixed"):
        a, r = A[f"seeds_only@{fixed}"], restated(f"seeds_only@{fixed}")
        assert r["nfound"] == 0 and (a["seed12"] >= 0).sum() >= 40 and r["opt"]["res"].nin >= 20           # the search finds nothing
        a, r = A[f"search_only@{fixed}"], restated(f"search_only@{fixed}")
        assert (a["seed12"] == -1).all() and r["nfound"] >= 60 and r["opt"]["res"].ncorrespondences == r["nfound"]
        a, r = A[f"both@{fixed}"], restated(f"both@{fixed}")
        assert (a["seed12"] >= 0).sum() >= 20 and r["nfound"] >= 40
        assert r["opt"]["res"].ncorrespondences == (a["seed12"] >= 0).sum() + r["nfound"]
        a, r = A[f"minus2@{fixed}"], restated(f"minus2@{fixed}")
        m2 = a["seed12"] == -2
        assert m2.sum() == 6 and (r["found12"][m2] == -1).all() and (r["matches12"][m2] == -2).all() and not np.isin(np.nonzero(m2)[0], r["idx"]).any()
        open_search = ref.cpu_search(dict(a, seed12=np.where(m2, -1, a["seed12"]).astype(np.int32)))[0]
        assert (open_search[m2] >= 0).all()                                  # unblocked, every one of those slots would have matched
        a, r = A[f"seed_invalid2@{fixed}"], restated(f"seed_invalid2@{fixed}")
        inv = (a["seed12"] >= 0) & (a["valid2"][np.maximum(a["seed12"], 0)] == 0)
        assert inv.sum() == 4 and not np.isin(np.nonzero(inv)[0], r["idx"]).any() and np.array_equal(r["matches12"][inv], a["seed12"][inv])
        a, r = A[f"seed_blocks@{fixed}"], restated(f"seed_blocks@{fixed}")
        robbed = [int(b) for b in range(a["family"]["n1"]) if a["partner"][b] >= 0 and a["seed12"][b] == -1 and
                  ((a["seed12"] == a["partner"][b]) & (np.arange(a["family"]["n1"]) != b)).any()]
        assert len(robbed) == 3 and (r["found12"][robbed] == -1).all()
        open_search = ref.cpu_search(dict(a, seed12=np.full_like(a["seed12"], -1)))[0]
        assert np.array_equal(open_search[robbed], a["partner"][robbed])     # without the seeds they match the keypoints the seeds took
        thieves = [int(np.nonzero(a["seed12"] == a["partner"][b])[0][0]) for b in robbed]
        assert (r["matches12"][thieves] == -1).all() and r["opt"]["res"].nbad >= 3                          # and the cut erases the wrong seeds
        r = restated(f"few@{fixed}")["opt"]["res"]
        assert r.ncorrespondences >= 10 and r.ncorrespondences - r.nbad < 10 and r.nin == 0 and r.iterations[1] == 0
        r = restated(f"none@{fixed}")
        assert r["nfound"] == 0 and r["opt"]["res"].ncorrespondences == 0 and A[f"none@{fixed}"]["n2"] > 100
    assert A["n2_zero"]["n2"] == 0 and restated("n2_zero")["opt"]["res"].ncorrespondences == 0
    big = restated("big@free")["opt"]["res"]
    assert 560 <= A["big@free"]["family"]["n1"] <= 640 and big.ncorrespondences > 512 and big.nin > 400      # SO_LDS_PAIRS' far path
    B = scenes.batches()
    assert all(150 <= a["family"]["n1"] <= 300 and a["n2"] <= 300 for n, a in A.items() if n != "big@free")
    assert len({a["n2"] for a in B["ragged3"][1]}) == 3 and len(B["p64"][1]) == 64 and len(B["big"][1]) == 1
    assert {a["shape"] for a in B["p64"][1]} >= set(scenes.SMALL) | {"n2_zero"}
    # the batch for the fold: its first attempt is planted to fail
    assert restated(B["ragged3"][1][1]["name"])["opt"]["res"].nin < s3.REFINE_MIN_INLIERS <= restated(B["ragged3"][1][2]["name"])["opt"]["res"].nin


def test_the_walk_is_the_reference_loop():
    """the numpy gather against a literal transcription of Optimizer.cc:1483-1520 over pointer-like lists"""
    a = attempts()["minus2@free"]
    fam = a["family"]
    found = restated("minus2@free")["found12"]
    vpMatches1 = [None if (a["seed12"][i] == -1 and found[i] < 0) else ("mp2", int(a["seed12"][i]) if a["seed12"][i] != -1 else int(found[i]))
                  for i in range(fam["n1"])]
    edges = []
    for i in range(fam["n1"]):
        if not vpMatches1[i]:
            continue
        i2 = vpMatches1[i][1] if vpMatches1[i][1] >= 0 else -1             # GetIndexInKeyFrame: -2 has none
        if fam["valid1"][i] and i2 >= 0 and a["valid2"][i2]:
            edges.append(i)
    prob, idx = ref.gather(a, found)
    assert list(idx) == edges and prob["n"] == len(edges)
    assert np.array_equal(prob["obs1"][:, 0], fam["kps1"]["x"][idx]) and np.array_equal(prob["octave1"], fam["kps1"]["octave"][idx])


# ------------------------------------------------------------------------------------------------ 2. selection rule and sensitivity
def measure_sensitivity():
    """as tests/test_cpu_sim3_opt.py computes D_cpu, over the attempts with a correspondence: the largest relative difference of
    (q, t, s) to the unperturbed run under the 16 +-1 ulp patterns, and per scene what would put an integer at the rounding floor"""
    rows, D = [], 0.0
    for name, a in attempts().items():
        base = restated(name)
        prob = base["problem"]
        if prob["n"] == 0:
            continue
        import sim3_opt_oracle as so
        v0 = base["opt"]["res"].vec()
        d, moved = 0.0, 0
        for seed in ULP_SEEDS:
            o = so.optimize(prob, scenes.INV_SIGMA2, ulp_seed=seed)
            d = max(d, float(np.max(np.abs(o["res"].vec() - v0) / np.abs(v0))))
            moved += _ints(o["res"]) != _ints(base["opt"]["res"]) or not np.array_equal(o["kept"], base["opt"]["kept"])
        rows.append(dict(name=name, d=d, moved=moved, base=base["opt"]))
        D = max(D, d)
    for r in rows:
        cc = r["base"]["cut_chi"]
        r["near"] = int(np.sum(np.abs(cc[~np.isnan(cc)] - scenes.TH2) < M * D * scenes.TH2))
        r["small_rho"] = int(r["base"]["trace"].small_rho)
    return D, rows


def test_every_scene_passes_the_selection_rule_and_the_sensitivity_is_the_pinned_one():
    D, rows = measure_sensitivity()
    out = [r["name"] for r in rows if r["near"] or r["small_rho"] or r["moved"]]
    print("D %.3e" % D, "left out:", out)
    assert not out, out                                          # 0 of N left out
    gold = json.load(open(GOLDEN))
    assert gold["scenes"] == [r["name"] for r in rows] and gold["ulp_seeds"] == ULP_SEEDS
    assert gold["D_cpu"] / 2 <= D <= gold["D_cpu"] * 2, (D, gold["D_cpu"])
    assert 1e-10 < gold["D_cpu"] < 1e-6


def test_what_the_search_finds_are_the_planted_partners():
    """the scenes' matches are real ones: what SearchBySim3 finds is, with few exceptions, the keypoint that shows the same point"""
    for name, a in attempts().items():
        f = restated(name)["found12"]
        hit = f >= 0
        if hit.any():
            assert (a["partner"][hit] == f[hit]).mean() > 0.95, name


# ------------------------------------------------------------------------------------------------ 3. surfaces
@pytest.fixture(scope="module")
def so_path():
    return _lib.build()


def test_new_entry_points_are_declared_exported_and_bound(so_path):
    protos = _lib.prototypes()
    vp = C.c_void_p
    assert protos["orbm_refine_sim3_candidates"] == (C.c_int, [vp] * 6 + [C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, vp, vp])
    assert protos["orbm_debug_last_refine_sim3_waits"] == (C.c_int, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path]).decode()
    for name in ("orbm_refine_sim3_candidates", "orbm_debug_last_refine_sim3_waits"):
        assert f" T {name}\n" in out
    assert _lib.lib().orbx_abi_version() == 136


def test_struct_mirror_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_refine_sim3")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_refine_sim3.c"), "-o", exe])
    sizes, fields = {}, {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    m, name = s3._CRefineSim3Attempt, "orbm_refine_sim3_attempt"
    assert C.sizeof(m) == sizes[name]
    assert [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_] == fields[name]


def test_refusals_that_need_no_frame_come_before_any_launch(so_path):
    L = _lib.lib()
    arr = (s3._CRefineSim3Attempt * 65)()
    nf = np.full(65, -9, np.int32); res = (s3.Sim3OptResult * 65)()
    call = lambda P, kf1=None: L.orbm_refine_sim3_candidates(kf1, None, None, None, None, arr, P, 7.5, 95, 10.0, 0, _lib.ptr(nf), res)
    assert call(65) == ERR_UNSUPPORTED and b"64" in L.orbx_last_error()
    assert call(-1) == ERR_ARG
    assert call(1) == ERR_ARG                                    # no current keyframe
    assert call(0) == OK                                         # nothing to do: on any machine
    assert L.orbm_debug_last_refine_sim3_waits() == 0 and (nf == -9).all() and bytes(res) == bytes(len(bytes(res)))


def test_the_unit_leases_one_workspace_declared_with_its_initialiser():
    src = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_refine_sim3.hip")).read()
    assert len(re.findall(r"^\s*StagedCall\s+\w+\s*\{\};", src, re.M)) == 1 and "WorkspaceLease" not in src
    assert "atomicAdd" not in src and "atomic_fetch" not in src                     # the pair order is a prefix scan's
    case = open(os.path.join(ROOT, "tests", "test_gpu_refine_sim3_workspace.py")).read()
    assert "W.FILLS" in case and "fill_workspaces" in case and "refine_sim3_candidates" in case
    mk = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "Makefile")).read()
    assert "orbm_refine_sim3.hip" in mk and "-ffp-contract=off" in mk
    for unit, helper in (("orbm_sim3opt.hip", "struct Sim3OptDev"), ("orbm_search.hip", "struct FormCam"), ("orbm_refine_sim3.hip", "struct FormCam")):
        assert helper not in open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", unit)).read(), (unit, helper)


def build_smoke(tmp_path):
    _lib.build()
    exe = str(tmp_path / "refine_sim3_smoke")
    libdir = os.path.join(ROOT, "orb_slam2_e_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wno-reorder", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "refine_sim3_smoke.cpp"), "-o", exe,
                           "-L", libdir, "-lorbslam_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_wrapper_compiles_and_fails_loudly_without_a_device(tmp_path):
    """the program compiles against the headers and links; without a device it reports that no frame can be made and leaves"""
    import torch
    if torch.cuda.is_available():
        return                                                  # its device run is tests/test_gpu_refine_sim3.py's
    out = subprocess.run([build_smoke(tmp_path), "nodevice"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK nodevice" in out.stdout, out.stdout + out.stderr


def test_integration_shell_calls_the_declared_entry_points():
    """integration/LoopClosing_sim3_hip.cc cannot be compiled here (no OpenCV / g2o): the library calls it makes have the declared
    numbers of arguments, every ORBM_ / ORBX_ constant it names exists, and the documents list it; reference.patch does not know it"""
    import test_cpu_integration_shells as shells
    decl, header_text = shells._declarations()
    src = open(os.path.join(ROOT, "integration", "LoopClosing_sim3_hip.cc")).read()
    calls = [c for c in shells._calls(src) if c[0] in decl]
    assert ("orbm_refine_sim3_candidates", 13) in calls and decl["orbm_refine_sim3_candidates"] == 13
    assert all(decl[f] == n for f, n in calls), calls
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", shells._strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    body = hpp[hpp.index("inline int RefineSim3Candidates("):]
    assert ("orbm_refine_sim3_candidates", 13) in [c for c in shells._calls(body) if c[0] in decl]
    assert "HipRefineSim3Candidates" in shells._strip_comments(src)
    assert "LoopClosing_sim3_hip.cc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "LoopClosing_sim3_hip.cc" in open(os.path.join(ROOT, "integration", "README.md")).read()
    assert "HipRefineSim3Candidates" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
