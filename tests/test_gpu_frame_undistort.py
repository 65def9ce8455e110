"""Resident frames straight from the extractor on a distorted camera, and batches of them, on the device:
  points   orbm_undistort_points against the numpy restatement (tests/undistort_reference.py), bit for bit where finite;
  single   orbm_frame_from_extractor_cam == orbm_frame_from_extractor fed orbm_undistort_points of the downloaded keypoints
           (equality a), one host wait against two, cam NULL / k1 == 0 == the existing entry, keypoints_un of a frame without a
           camera == the extractor's coordinates (equality c);
  batch    orbm_frames_from_extractor == the single calls (equality b), one wait, all-or-nothing refusals;
  stereo   the batch with uright_from_stereo == the single calls;
  C++      the ResidentFrame forms give the bytes Python gets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import undistort_reference as ur
from orb_slam2_e_amd import (Distortion, Frame, ORBextractor, ORBmatcher, extract_pair, image_bounds, stereo_download_batch, stereo_match_batch,
                             undistort_points)
from orb_slam2_e_amd._lib import lib, ptr as _p
from orb_slam2_e_amd.synth import synth_frame, synth_stereo_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
ERR_ARG, ERR_CAPACITY = -1, -4
GRID_COLS, GRID_ROWS = 64, 48
NAMES = sorted(ur.CAMERAS)
HAM = ur.CAMERAS["sHamlyn04"][0]
PRM = (500, 1.2, 8, 20, 7)
NARROW = (40.0, 30.0, 600.0, 450.0)
M = ORBmatcher(0.6)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cells(xy, bounds):
    """Frame::PosInGrid restated: the cell (col * 48 + row) of float32 coordinates, -1 outside the grid (also not finite ones)."""
    f32 = np.float32
    inv_w = f32(GRID_COLS) / (f32(bounds[2]) - f32(bounds[0])); inv_h = f32(GRID_ROWS) / (f32(bounds[3]) - f32(bounds[1]))
    out = []
    with np.errstate(all="ignore"):
        for v, lo, inv in ((xy[:, 0], bounds[0], inv_w), (xy[:, 1], bounds[1], inv_h)):
            t = ((v.astype(f32) - f32(lo)) * inv).astype(np.float64)            # the float product, then roundf: half away from zero
            out.append(np.where(t >= 0, np.floor(t + 0.5), np.ceil(t - 0.5)))
    px, py = out
    inside = np.isfinite(px) & np.isfinite(py) & (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    return np.where(inside, np.nan_to_num(px) * GRID_ROWS + np.nan_to_num(py), -1).astype(np.int64)


def same_frame(a, b):
    """equalities (a) / (b): size, layout and the coordinates the searches use"""
    pa, ca = a.layout(); pb, cb = b.layout()
    return (a.n, a.ns) == (b.n, b.ns) and np.array_equal(pa, pb) and np.array_equal(ca, cb) and np.array_equal(bits(a.keypoints_un()), bits(b.keypoints_un()))


def window_queries(rng, xy, desc, nq=50, stereo=False):
    """nq windows around keypoints of the frame (finite centres), every level"""
    ok = np.nonzero(np.isfinite(xy).all(1))[0]
    pick = rng.choice(ok, nq)
    q = np.zeros(nq, ORBmatcher.WQ_DTYPE)
    q["u"] = xy[pick, 0] + rng.uniform(-6, 6, nq); q["v"] = xy[pick, 1] + rng.uniform(-6, 6, nq)
    q["r"] = rng.uniform(8, 30, nq); q["min_level"] = 0; q["max_level"] = -1
    q["xr"] = np.where(rng.random(nq) < 0.5, q["u"] - rng.uniform(2, 40, nq), -1.0) if stereo else 0.0
    return q, np.ascontiguousarray(desc[rng.permutation(pick)])


def same_search(q, qd, a, b):
    ra, rb = M.frame_search_window(a, q, qd), M.frame_search_window(b, q, qd)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    return ra


# ------------------------------------------------------------------------------------------------ points

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
@pytest.mark.parametrize("name", NAMES)
def test_points_equal_the_restatement(name, n):
    cam, size = ur.CAMERAS[name]
    pts = ur.sample_points(cam, size, n)
    assert len(pts) == n
    got = undistort_points(Distortion(*cam), pts)
    want = ur.undistort(cam, pts)
    assert ur.same_bits_or_both_not_finite(got, want)
    if n:
        buf = pts.copy()                                                      # in place: xy_un == xy
        assert lib().orbm_undistort_points(C.byref(Distortion(*cam)), _p(buf), n, _p(buf)) == 0
        assert ur.same_bits_or_both_not_finite(buf, want)
    if n == 1025:
        moved = (bits(got) != bits(pts)).any(1).sum()
        assert moved >= n - 2                                                 # (the principal point of a camera may stay)
        if name == "sHCULB_00053":                                            # the divergence branch is reached on the device too
            with np.errstate(all="ignore"):
                shift = np.hypot(got[:, 0].astype(np.float64) - pts[:, 0], got[:, 1].astype(np.float64) - pts[:, 1])
            assert (shift[np.isfinite(shift)] > 1000).any()


def test_points_with_k1_zero_come_back_as_they_are():
    cam = list(HAM); cam[4] = 0.0
    pts = ur.sample_points(cam, (640, 480), 65)
    assert np.array_equal(bits(undistort_points(Distortion(*cam), pts)), bits(pts))


# ------------------------------------------------------------------------------------------------ single frame

@pytest.fixture(scope="module")
def one():
    ex = ORBextractor(*PRM)
    kps, desc = ex(synth_frame(3))
    assert len(kps) > 300
    return ex, kps, desc, np.ascontiguousarray(np.stack([kps["x"], kps["y"]], 1), np.float32)


@pytest.mark.parametrize("which", ["corner bounds", "narrower bounds"])
def test_camera_form_equals_the_host_undistortion_form(one, which):
    """Equality (a) under sHamlyn04, with the layout also checked against the host sort of the restated coordinates."""
    ex, kps, desc, xy = one
    cam = Distortion(*HAM)
    bounds = image_bounds(cam, 640, 480) if which == "corner bounds" else NARROW
    want = ur.undistort(HAM, xy)
    c_before, c_after = cells(xy, bounds), cells(want, bounds)
    assert ((c_before != c_after) & (c_before >= 0) & (c_after >= 0)).any()            # a keypoint changes its cell through undistortion
    outside = int((c_after < 0).sum())
    assert (cells(want, NARROW) < 0).any()                                              # ... and one lies outside the (narrower) grid
    xy_un = undistort_points(cam, xy)
    assert ur.same_bits_or_both_not_finite(xy_un, want)
    a = Frame.from_extractor(ex, 0, bounds, camera=cam); waits_a = Frame.last_build_waits()
    b = Frame.from_extractor(ex, 0, bounds, xy_undistorted=xy_un); waits_b = Frame.last_build_waits()
    assert (waits_a, waits_b) == (1, 2)
    assert same_frame(a, b)
    assert a.n == len(kps) and a.n - a.ns == outside
    assert np.array_equal(bits(a.keypoints_un()), bits(xy_un))
    # the device-built order against the host counting sort of the restated coordinates
    k2 = kps.copy(); k2["x"] = want[:, 0]; k2["y"] = want[:, 1]
    perm = np.zeros(len(kps), np.int32); cell_off = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32); ns = C.c_int(0)
    assert lib().orbm_sorted_frame(_p(k2), len(k2), None, None, *[float(v) for v in bounds], _p(perm), _p(cell_off), C.byref(ns)) == 0
    assert ns.value == a.ns and np.array_equal(perm[:a.ns], a.layout()[0]) and np.array_equal(cell_off, a.layout()[1])
    q, qd = window_queries(np.random.default_rng(5), want, desc)
    res = same_search(q, qd, a, b)
    assert (res[4] >= 0).sum() > 25
    # with a host uright array the count is read back first: two waits, same frame
    urt = np.where(np.arange(len(kps)) % 3 == 0, xy[:, 0] - 7.5, -1.0).astype(np.float32)
    c = Frame.from_extractor(ex, 0, bounds, camera=cam, uright=urt); waits_c = Frame.last_build_waits()
    d = Frame.from_extractor(ex, 0, bounds, xy_undistorted=xy_un, uright=urt)
    assert waits_c == 2 and same_frame(c, d) and same_frame(c, a)
    q, qd = window_queries(np.random.default_rng(6), want, desc, stereo=True)
    same_search(q, qd, c, d)
    for f in (a, b, c, d):
        f.close()


def test_no_camera_and_k1_zero_equal_the_existing_entry(one):
    """cam = NULL and k1 == 0 (with k2 != 0) are the existing entry with xy_undistorted = NULL; equality (c)."""
    ex, kps, desc, xy = one
    bounds = (0.0, 0.0, 640.0, 480.0)
    old = Frame.from_extractor(ex, 0, bounds)
    assert Frame.last_build_waits() == 1
    h = C.c_void_p()
    assert lib().orbm_frame_from_extractor_cam(ex._h, 0, None, None, 0, *bounds, C.byref(h)) == 0
    null = Frame(bounds=bounds, _handle=h)
    assert Frame.last_build_waits() == 1
    cam0 = list(HAM); cam0[4] = 0.0
    assert cam0[5] != 0
    zero = Frame.from_extractor(ex, 0, bounds, camera=Distortion(*cam0))
    assert same_frame(null, old) and same_frame(zero, old)
    assert np.array_equal(bits(old.keypoints_un()), bits(xy))                 # (c): the extractor's own coordinates
    q, qd = window_queries(np.random.default_rng(7), xy, desc)
    same_search(q, qd, zero, old)
    for f in (old, null, zero):
        f.close()


def test_refusals_come_before_any_device_work(one):
    ex = one[0]
    L = lib()
    good = Distortion(*HAM)
    b = (0.0, 0.0, 640.0, 480.0)
    hs = (C.c_void_p * 4)()
    h = C.c_void_p()
    urt = np.zeros(ex.capacity, np.float32)

    def batch(first=0, count=1, cam=good, stereo=0, bounds=b, out=hs):
        return L.orbm_frames_from_extractor(ex._h, first, count, C.byref(cam) if cam is not None else None, stereo, *bounds, out)

    def single(frame=0, cam=good, uright=None, stereo=0, bounds=b, out=C.byref(h)):
        return L.orbm_frame_from_extractor_cam(ex._h, frame, C.byref(cam) if cam is not None else None, uright, stereo, *bounds, out)

    assert batch(first=-1) == ERR_ARG and batch(count=-1) == ERR_ARG and batch(first=1) == ERR_ARG and batch(count=2) == ERR_ARG
    assert batch(first=2**31 - 1, count=2**31 - 1) == ERR_ARG
    assert batch(bounds=(0.0, 0.0, 0.0, 480.0)) == ERR_ARG and batch(bounds=(0.0, 480.0, 640.0, 480.0)) == ERR_ARG
    assert batch(bounds=(0.0, 0.0, float("nan"), 480.0)) == ERR_ARG and batch(out=None) == ERR_ARG
    assert batch(stereo=1) == ERR_ARG                                          # no orbx_stereo_match ran on this handle
    assert single(frame=-1) == ERR_ARG and single(frame=1) == ERR_ARG and single(out=None) == ERR_ARG
    assert single(bounds=(640.0, 0.0, 0.0, 480.0)) == ERR_ARG and single(uright=_p(urt), stereo=1) == ERR_ARG
    for i in range(9):
        for v in (float("nan"), float("inf")):
            c = list(HAM); c[i] = v
            assert batch(cam=Distortion(*c)) == ERR_ARG and single(cam=Distortion(*c)) == ERR_ARG
    for i in (0, 1):
        c = list(HAM); c[i] = 0.0
        assert batch(cam=Distortion(*c)) == ERR_ARG and single(cam=Distortion(*c)) == ERR_ARG
    assert not h.value and not any(hs)
    assert batch(count=0) == 0 and not any(hs) and Frame.last_build_waits() == 0      # nothing launched, nothing waited for
    big = ORBextractor(9000, 1.2, 8, 20, 7)                                   # more than 8,192 keypoints per frame, as today
    big(synth_frame(0))
    assert big.capacity > 8192
    assert L.orbm_frames_from_extractor(big._h, 0, 1, None, 0, *b, hs) == ERR_CAPACITY
    assert L.orbm_frame_from_extractor_cam(big._h, 0, C.byref(good), None, 0, *b, C.byref(h)) == ERR_CAPACITY
    assert not h.value and not any(hs)


# ------------------------------------------------------------------------------------------------ batch

@pytest.fixture(scope="module")
def five():
    """five different images, the third blank (0 keypoints); the single-call handles of every frame, with and without the camera"""
    imgs = np.stack([synth_frame(0), synth_frame(1), np.full((480, 640), 128, np.uint8), synth_frame(2), synth_frame(4)])
    ex = ORBextractor(*PRM)
    ex.extract_batch(imgs)
    cam = Distortion(*HAM)
    bounds = {None: (0.0, 0.0, 640.0, 480.0), "cam": NARROW}
    singles = {key: [Frame.from_extractor(ex, f, bounds[key], camera=cam if key else None) for f in range(5)] for key in bounds}
    assert singles[None][2].n == 0 and all(singles[None][f].n > 300 for f in (0, 1, 3, 4))
    perms = [singles[None][f].layout()[0].tobytes() for f in (0, 1, 3, 4)]
    assert len(set(perms)) == 4                                              # (a batch that mixed frames up would not pass for right)
    assert any(s.n > s.ns for s in singles["cam"])
    return ex, cam, bounds, singles


@pytest.mark.parametrize("key", [None, "cam"])
@pytest.mark.parametrize("first,count", [(0, 1), (2, 1), (0, 2), (2, 2), (0, 5)])
def test_batch_equals_the_single_calls(five, first, count, key):
    """Equality (b): out[i] of the batch call equals the single call for frame first + i; one wait for the whole batch."""
    ex, cam, bounds, singles = five
    frames = Frame.batch_from_extractor(ex, first, count, bounds[key], camera=cam if key else None)
    assert Frame.last_build_waits() == 1 and len(frames) == count
    for i, f in enumerate(frames):
        assert same_frame(f, singles[key][first + i]), (first, i)
    again = Frame.batch_from_extractor(ex, first, count, bounds[key], camera=cam if key else None)      # the same call twice
    for f, g in zip(frames, again):
        assert same_frame(f, g)
    for f in frames + again:
        f.close()


def test_batch_past_the_last_frame_is_refused_and_writes_nothing(five):
    ex, cam, bounds, _ = five
    hs = (C.c_void_p * 6)()
    assert lib().orbm_frames_from_extractor(ex._h, 2, 5, C.byref(cam), 0, *bounds["cam"], hs) == ERR_ARG and not any(hs)
    assert lib().orbm_frames_from_extractor(ex._h, 0, 6, C.byref(cam), 0, *bounds["cam"], hs) == ERR_ARG and not any(hs)


def test_handles_of_a_batch_are_independent(five):
    """Destroyed in another order than made; a search through a surviving handle is still right."""
    ex, cam, bounds, singles = five
    frames = Frame.batch_from_extractor(ex, 0, 5, bounds["cam"], camera=cam)
    for i in (3, 0, 4, 2):
        frames[i].close()
    fresh = Frame.batch_from_extractor(ex, 3, 2, bounds["cam"], camera=cam)      # takes recycled blocks while frames[1] lives
    kps, desc = ex.download(1)
    xy_un = frames[1].keypoints_un()
    assert np.array_equal(bits(xy_un), bits(singles["cam"][1].keypoints_un()))
    q, qd = window_queries(np.random.default_rng(9), xy_un, desc)
    res = same_search(q, qd, frames[1], singles["cam"][1])
    assert (res[4] >= 0).sum() > 25
    assert same_frame(fresh[0], singles["cam"][3]) and same_frame(fresh[1], singles["cam"][4])
    for f in [frames[1]] + fresh:
        f.close()


# ------------------------------------------------------------------------------------------------ stereo

def test_stereo_batch_equals_the_single_calls():
    """Two pairs through orbx_extract_pair / orbx_stereo_match, then two pairs as one batch: with uright_from_stereo the batch call
    equals the single calls, in layout, coordinates and a stereo-checked window search."""
    prm = (800, 1.2, 8, 20, 7)
    eL, eR = ORBextractor(*prm), ORBextractor(*prm)
    mbf = np.float32(40.0); mb = mbf / np.float32(500.0)
    cam = Distortion(*HAM)
    pairs = [synth_stereo_pair(k, 640, 480) for k in (1, 2)]
    for left, right in pairs:
        (kps, desc), _ = extract_pair(eL, eR, left, right)
        stereo_match_batch(eL, eR, mb, mbf)
        eL._last_B = 1
        assert (stereo_download_batch(eL)[0][0, :len(kps)] >= 0).sum() > 50       # (as every caller so far: the match has finished)
        one = Frame.from_extractor(eL, 0, NARROW, camera=cam, uright_from_stereo=True)
        assert Frame.last_build_waits() == 1
        got = Frame.batch_from_extractor(eL, 0, 1, NARROW, camera=cam, uright_from_stereo=True)[0]
        assert Frame.last_build_waits() == 1
        mono = Frame.from_extractor(eL, 0, NARROW, camera=cam)
        assert same_frame(got, one) and same_frame(mono, one)
        q, qd = window_queries(np.random.default_rng(12), one.keypoints_un(), desc, stereo=True)
        stereo_res = same_search(q, qd, got, one)
        mono_res = M.frame_search_window(mono, q, qd)
        assert not all(np.array_equal(x, y) for x, y in zip(stereo_res, mono_res))     # the right coordinates are really in the handle
        for f in (one, got, mono):
            f.close()
    eL.extract_batch(np.stack([p[0] for p in pairs])); eR.extract_batch(np.stack([p[1] for p in pairs]))
    stereo_match_batch(eL, eR, mb, mbf)
    stereo_download_batch(eL)
    got = Frame.batch_from_extractor(eL, 0, 2, NARROW, camera=cam, uright_from_stereo=True)
    assert Frame.last_build_waits() == 1
    for f in range(2):
        one = Frame.from_extractor(eL, f, NARROW, camera=cam, uright_from_stereo=True)
        assert same_frame(got[f], one)
        q, qd = window_queries(np.random.default_rng(13 + f), one.keypoints_un(), eL.download(f)[1], stereo=True)
        same_search(q, qd, got[f], one)
        one.close(); got[f].close()


# ------------------------------------------------------------------------------------------------ C++

def test_cxx_forms_give_the_bytes_python_gets(five, tmp_path):
    """orbslam_hip::ORBmatcher::ResidentFrame's camera constructor, FromBatch and KeysUn (tests/cxx/frame_forms.cpp) on the five
    images: sizes, permutations and mvKeysUn coordinates of the Python handles."""
    _, cam, bounds, singles = five
    exe = str(tmp_path / "frame_forms")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "frame_forms.cpp"),
                           "-o", exe, "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    imgs = np.stack([synth_frame(0), synth_frame(1), np.full((480, 640), 128, np.uint8), synth_frame(2), synth_frame(4)])
    with open(tmp_path / "scene.bin", "wb") as f:
        f.write(np.array([5, 480, 640, PRM[0]], np.int32).tobytes())
        f.write(np.array(HAM, np.float32).tobytes() + np.array(bounds["cam"], np.float32).tobytes())
        f.write(imgs.tobytes())
    out = subprocess.run([exe, str(tmp_path / "scene.bin"), str(tmp_path / "frames.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    data = np.fromfile(tmp_path / "frames.bin", np.int32)
    at = 0
    for frame in [0, 0, 1, 2, 3, 4]:                                          # the constructor form, then FromBatch(0, 5)
        s = singles["cam"][frame]
        n, ns = data[at], data[at + 1]
        assert (n, ns) == (s.n, s.ns)
        assert np.array_equal(data[at + 2:at + 2 + ns], s.layout()[0])
        assert np.array_equal(data[at + 2 + ns:at + 2 + ns + 2 * n].view(np.uint32), bits(s.keypoints_un()).reshape(-1))
        at += 2 + ns + 2 * n
    assert at == len(data)
