"""Frame::UndistortKeyPoints / ComputeImageBounds and the frame-making entries that take a camera, without a GPU: the new symbols
are declared, exported and bound and orbm_distortion has the C layout; orbm_image_bounds (host only) equals the numpy restatement
(tests/undistort_reference.py) bit for bit; the restatement inverts the forward distortion model; every refusal happens before the
device is needed and writes nothing; integration/hip_frame.h calls only what the headers declare."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import undistort_reference as ur
from orb_slam2_e_amd import Distortion, Frame, OrbxError, image_bounds, undistort_points
from orb_slam2_e_amd._lib import lib, prototypes, ptr as _p
from test_cpu_integration_shells import _calls, _declarations, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
NEW = {"orbm_image_bounds": 4, "orbm_undistort_points": 4, "orbm_frame_from_extractor_cam": 10, "orbm_frames_from_extractor": 10,
       "orbm_frame_keypoints_un": 2, "orbm_debug_last_frame_build_waits": 0}
ERR_ARG, ERR_NO_DEVICE = -1, -2
NAMES = sorted(ur.CAMERAS)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_new_symbols_are_declared_exported_and_bound():
    protos = prototypes()
    L = lib()
    for name, nargs in NEW.items():
        assert name in protos and len(protos[name][1]) == nargs, name
        assert getattr(L, name).argtypes == protos[name][1]
    assert L.orbx_abi_version() == 136
    for name in ("from_extractor", "batch_from_extractor", "keypoints_un", "last_build_waits"):
        assert callable(getattr(Frame, name))
    assert Frame.last_build_waits() in (0, 1, 2)
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    for word in ("struct Distortion", "ImageBounds", "FromBatch", "KeysUn", "orbm_frame_from_extractor_cam", "orbm_frames_from_extractor"):
        assert word in hpp, word


def test_distortion_mirror_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "abi_layout_distortion")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout_distortion.c"), "-o", exe])
    lines = [l.split() for l in subprocess.check_output([exe]).decode().splitlines()]
    assert lines[0] == ["struct", "orbm_distortion", str(C.sizeof(Distortion))]
    fields = [(w[2], int(w[3]), int(w[4])) for w in lines[1:]]
    assert fields == [(f[0], getattr(Distortion, f[0]).offset, getattr(Distortion, f[0]).size) for f in Distortion._fields_]
    assert [f[0] for f in fields] == ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"]


@pytest.mark.parametrize("name", NAMES)
def test_image_bounds_equal_the_restatement_bit_for_bit(name):
    cam, (w, h) = ur.CAMERAS[name]
    got = np.array(image_bounds(Distortion(*cam), w, h), np.float32)
    want = ur.image_bounds(cam, w, h)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert got[0] < got[2] and got[1] < got[3] and not np.array_equal(got, np.array([0, 0, w, h], np.float32))


def test_k1_zero_means_no_undistortion_whatever_k2_is():
    for name in NAMES:
        cam, (w, h) = ur.CAMERAS[name]
        cam = list(cam); cam[4] = 0.0
        assert cam[5] != 0
        assert image_bounds(Distortion(*cam), w, h) == (0.0, 0.0, float(w), float(h))
        assert np.array_equal(ur.image_bounds(cam, w, h), np.array([0, 0, w, h], np.float32))
        pts = ur.sample_points(cam, (w, h), 65)
        assert np.array_equal(ur.undistort(cam, pts), pts)


def test_the_restatement_inverts_the_forward_model():
    """First principles: the normalised result pushed through the forward distortion model returns to the input pixel within
    1e-2 px on 5,000 uniform points of the sHamlyn04 image (20 x the 4.9e-4 px measured on the CPU)."""
    cam, (w, h) = ur.CAMERAS["sHamlyn04"]
    rng = np.random.default_rng(11)
    pts = (rng.random((5000, 2)) * [w, h]).astype(np.float32)
    x, y = ur.normalised(cam, pts)
    u, v = ur.distort(cam, x, y)
    err = np.hypot(u - pts[:, 0].astype(np.float64), v - pts[:, 1].astype(np.float64))
    print("largest return error [px]:", err.max())
    assert err.max() < 1e-2


def test_the_wide_angle_camera_has_diverging_points():
    """The precondition of the divergence branch, on the restatement alone: on the sHCULB_00053 camera at least one point of its
    720 x 540 image moves by more than 1,000 px."""
    cam, (w, h) = ur.CAMERAS["sHCULB_00053"]
    pts = ur.sample_points(cam, (w, h), 1025)
    out = ur.undistort(cam, pts).astype(np.float64)
    shift = np.hypot(out[:, 0] - pts[:, 0], out[:, 1] - pts[:, 1])
    print("largest shift [px]:", np.nanmax(shift), "not finite:", int((~np.isfinite(shift)).sum()))
    assert (shift[np.isfinite(shift)] > 1000).any()


def _bad_cameras():
    cam = ur.CAMERAS["sHamlyn04"][0]
    out = []
    for i in range(9):
        for v in (np.nan, np.inf, -np.inf):
            c = list(cam); c[i] = v
            out.append(c)
    for i in (0, 1):
        c = list(cam); c[i] = 0.0
        out.append(c)
    return out


def test_image_bounds_refusals_write_nothing():
    L = lib()
    good = Distortion(*ur.CAMERAS["sHamlyn04"][0])
    b = np.full(4, -7, np.float32)
    assert L.orbm_image_bounds(None, 640, 480, _p(b)) == ERR_ARG
    assert L.orbm_image_bounds(C.byref(good), 640, 480, None) == ERR_ARG
    assert L.orbm_image_bounds(C.byref(good), 0, 480, _p(b)) == ERR_ARG and L.orbm_image_bounds(C.byref(good), 640, -1, _p(b)) == ERR_ARG
    for c in _bad_cameras():
        assert L.orbm_image_bounds(C.byref(Distortion(*c)), 640, 480, _p(b)) == ERR_ARG, c
        assert lib().orbx_last_error()
    assert (b == -7).all()
    with pytest.raises(OrbxError):
        image_bounds(Distortion(0.0, 1.0, 0.0, 0.0, -0.1), 640, 480)


def test_device_entries_refuse_before_the_device_is_needed_and_write_nothing():
    L = lib()
    good = Distortion(*ur.CAMERAS["sHamlyn04"][0])
    xy = np.full((8, 2), 3.0, np.float32); out = np.full((8, 2), -7, np.float32)
    assert L.orbm_undistort_points(None, _p(xy), 8, _p(out)) == ERR_ARG
    assert L.orbm_undistort_points(C.byref(good), _p(xy), -1, _p(out)) == ERR_ARG
    assert L.orbm_undistort_points(C.byref(good), None, 8, _p(out)) == ERR_ARG
    assert L.orbm_undistort_points(C.byref(good), _p(xy), 8, None) == ERR_ARG
    for c in _bad_cameras():
        assert L.orbm_undistort_points(C.byref(Distortion(*c)), _p(xy), 8, _p(out)) == ERR_ARG, c
    assert (out == -7).all()
    # the frame-making entries: no extractor, nowhere to put the handle
    h = C.c_void_p(); hs = (C.c_void_p * 2)()
    assert L.orbm_frame_from_extractor_cam(None, 0, C.byref(good), None, 0, 0.0, 0.0, 640.0, 480.0, C.byref(h)) == ERR_ARG and not h.value
    assert L.orbm_frames_from_extractor(None, 0, 2, C.byref(good), 0, 0.0, 0.0, 640.0, 480.0, hs) == ERR_ARG and not hs[0] and not hs[1]
    assert L.orbm_frames_from_extractor(None, 0, 0, None, 0, 0.0, 0.0, 640.0, 480.0, hs) == ERR_ARG
    xyo = np.full(4, -7, np.float32)
    assert L.orbm_frame_keypoints_un(None, _p(xyo)) == ERR_ARG and (xyo == -7).all()


def test_without_a_device_the_device_entries_fail_loudly():
    if not _no_gpu():
        pytest.skip("GPU present")
    L = lib()
    good = Distortion(*ur.CAMERAS["sHamlyn04"][0])
    xy = np.full((8, 2), 3.0, np.float32); out = np.full((8, 2), -7, np.float32)
    assert L.orbm_undistort_points(C.byref(good), _p(xy), 8, _p(out)) == ERR_NO_DEVICE and (out == -7).all()
    assert L.orbm_undistort_points(C.byref(good), None, 0, None) == ERR_NO_DEVICE      # (arguments first, then the device)
    with pytest.raises(OrbxError) as e:
        undistort_points(good, xy)
    assert e.value.code == ERR_NO_DEVICE


def test_cxx_forms_compile_and_fail_loudly_without_a_device(tmp_path):
    if not _no_gpu():
        pytest.skip("GPU present")
    exe = str(tmp_path / "frame_forms")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "frame_forms.cpp"),
                           "-o", exe, "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "nodevice"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK nodevice" in out.stdout, out.stdout + out.stderr


def test_frame_shell_calls_only_declared_entry_points():
    """integration/hip_frame.h cannot be compiled here (no OpenCV): the calls it makes exist with the declared arity, the overload that
    takes mK / mDistCoef makes the handle with the camera entry and fills mvKeysUn from the handle, and the way the Frame constructor
    reaches it is described, not patched (integration/reference.patch stays as it is)."""
    decl, header_text = _declarations()
    L = lib()
    src = open(os.path.join(ROOT, "integration", "hip_frame.h")).read()
    called = set()
    for fn, nargs in _calls(src):
        if fn not in decl:
            assert re.search(r"\b%s\b" % fn, header_text), f"{fn} is not in include/*.h"     # a type name in a cast or an initialiser
            continue
        assert decl[fn] == nargs, f"{fn} called with {nargs} arguments, declared with {decl[fn]}"
        assert hasattr(L, fn)
        called.add(fn)
    assert called == {"orbm_frame_from_extractor", "orbm_frame_from_extractor_cam", "orbm_frame_keypoints_un", "orbm_frame_size",
                      "orbm_image_bounds", "orbm_frame_alias", "orbm_frame_destroy"}
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", _strip_comments(src))):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    code = _strip_comments(src)
    assert len(re.findall(r"\bHipFramePtr HipFrameFromExtractor\(", code)) == 2 and "HipImageBounds" in code
    for doc in ("INTEGRATION.md", os.path.join("integration", "README.md")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "orbm_frame_from_extractor_cam" in text and "HipImageBounds" in text, doc
    assert "_cam" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
