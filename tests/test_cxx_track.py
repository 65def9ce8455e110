"""orbslam_hip::ORBmatcher::TrackWithMotionModel / TrackLocalMap (include/orbslam_hip.hpp) from C++ (tests/cxx/track_smoke.cpp):
with a device each one-call result equals the search followed by PoseOptimization; without one the calls fail loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")


def _build(tmp_path):
    from orb_slam2_e_amd import _lib
    _lib.build()
    exe = str(tmp_path / "track_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "track_smoke.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_tracking_calls_compile_and_fail_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = _build(tmp_path)
    out = subprocess.run([exe, "nodevice"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK nodevice" in out.stdout


@pytest.mark.gpu
def test_cxx_tracking_calls_equal_search_then_pose(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK")
