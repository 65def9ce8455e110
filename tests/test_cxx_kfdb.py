"""orbslam_hip::KeyFrameDatabase (include/orbslam_hip.hpp) from C++ (tests/cxx/kfdb_host.cpp): with a device, its candidates, its
minScore and its six persistent fields over sequences of adds, erases, a clear and both kinds of query are those of
tests/kfdb_oracle.cc, fed the same case; without one the first add fails loudly."""
import os
import subprocess

import numpy as np
import pytest

import kfdb_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")


def _build(tmp_path):
    from orb_slam2_e_amd import _lib
    _lib.lib()                                       # (builds the library if it is missing)
    exe = str(tmp_path / "kfdb_host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "kfdb_host.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _case(seed, **kw):
    ops = []
    for op in S.sequence(seed, **kw):
        if op[0] == "loop":
            ops.append(("score", op[1], op[3]))        # DetectLoop's minScore loop over the connected slots ...
        ops.append(op)
    return ops


def test_cxx_kfdb_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = _build(tmp_path)
    out = subprocess.run([exe], input=S.case_text(1000, S.sequence(1)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and out.stdout == "NODEVICE\n", out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("seed, kw", [(31, dict(nkf=60, nqueries=10, words=80)), (32, dict(clear_at=4))])
def test_cxx_kfdb_gives_the_oracles_candidates_and_fields(seed, kw, tmp_path):
    exe = _build(tmp_path)
    # ... of which only the live ones may be listed: the case is made against the restatement's bookkeeping
    ops, alive = [], []
    for op in _case(seed, **kw):
        if op[0] == "add":
            alive.append(True)
        elif op[0] == "erase":
            alive[op[1]] = False
        elif op[0] == "clear":
            alive = []
        elif op[0] == "score":
            op = ("score", op[1], [s for s in op[2] if alive[s]])
        ops.append(op)
    text = S.case_text(1000, ops)
    want = S.run_oracle(S.build_oracle(tmp_path), text)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.endswith("OK\n"), out.stdout[-400:] + out.stderr
    got = S.parse_output(out.stdout[:-3])
    assert [r[0] for r in got] == [r[0] for r in want]
    ncand = 0
    for g, w in zip(got, want):
        if g[0] == "A":
            assert g == w
        elif g[0] == "S":
            assert S.same_bits(g[1], [min([np.float32(1)] + list(w[1]))])
        elif g[0] == "F":
            for a, b in zip(g[1], w[1]):
                assert S.same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
        else:
            assert g[1] == w[1]
            ncand += len(g[1])
    assert ncand > 0
