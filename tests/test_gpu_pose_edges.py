"""The device PoseOptimization (orbm_pose.hip) at its edges: the device-array batch form, the kernel's limits (a thread owns
keypoints t, t + 256, ... with one mask bit each; the first 1,024 keypoints are staged in LDS, the rest fetched from global
memory; at most 8,192 keypoints and 32 levels), the resident-frame and C++ forms on frames the other tests do not build, and an
optimality check of the result that does not go through the CPU restatement (tests/pose_optimum.py).

Comparisons with the restatement use the margins and the bar of tests/test_gpu_pose.py; the forms are compared with each other bit
for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import pose_only_oracle as po
import pose_only_scene as ps
import pose_optimum as pm
from orb_slam2_e_amd import ORBextractor, pose_optimization, pose_optimization_batch, pose_optimization_batch_device
from orb_slam2_e_amd._lib import SO_PATH, lib
from orb_slam2_e_amd.matcher import Frame
from orb_slam2_e_amd.pose import PoseStats, _camera, _kps
from orb_slam2_e_amd.synth import synth_frame
from test_gpu_pose import _agree, _margins_ok, _ulp_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -5
STATS_BYTES = C.sizeof(PoseStats)


def _dev(p, frame=None):
    return pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"], p["Tcw"],
                             frame=frame)


def _same(a, b, hm):
    """two (ngood, Tcw_out, outlier, stats) results: equal bits (outlier flags where has_mp)"""
    assert a[0] == b[0]
    bits = [np.asarray(x[1], np.float32).reshape(16).view(np.uint32) for x in (a, b)]
    assert np.array_equal(bits[0], bits[1])
    assert np.array_equal(a[2][hm], b[2][hm])
    assert bytes(a[3]) == bytes(b[3])


# ------------------------------------------------------------------------------------------------ A. the device-array batch form

def _to_dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).reshape(-1).copy()).cuda()


def _device_batch(problems, uright=True, stats=True, stream=None, sentinel=0xAA):
    """orbm_pose_optimization_batch(is_device = 1) on torch device tensors.  Outputs are pre-filled with `sentinel` bytes.
    Returns (ngood int32[B], Tout float32[B, 16], outlier uint8[total], stats uint8[B, STATS_BYTES] or None, kp_off)."""
    B = len(problems)
    sizes = [len(p["has_mp"]) for p in problems]
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    k = np.concatenate([_kps(p["kp_xy"], p["octave"]) for p in problems])
    ur = np.concatenate([np.full(s, -1, np.float32) if p["uright"] is None else np.asarray(p["uright"], np.float32)
                         for p, s in zip(problems, sizes)])
    has = np.concatenate([np.asarray(p["has_mp"], np.uint8) for p in problems])
    mp = np.concatenate([np.asarray(p["mp_pos"], np.float32).reshape(-1, 3) for p in problems])
    Tin = np.stack([np.asarray(p["Tcw"], np.float32).reshape(16) for p in problems])
    total = int(off[-1])
    d_k, d_ur, d_off = _to_dev(k), _to_dev(ur, np.float32), _to_dev(off, np.int32)
    d_has, d_mp, d_Tin = _to_dev(has), _to_dev(mp, np.float32), _to_dev(Tin, np.float32)
    d_Tout = torch.full((B * 16 * 4,), sentinel, dtype=torch.uint8, device="cuda")
    d_out = torch.full((max(total, 1),), sentinel, dtype=torch.uint8, device="cuda")
    d_ng = torch.full((B * 4,), sentinel, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B * STATS_BYTES,), sentinel, dtype=torch.uint8, device="cuda") if stats else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    pose_optimization_batch_device(d_k, d_ur if uright else None, d_off, B, d_has, d_mp, ps.CAM, problems[0]["inv_sigma2"], d_Tin,
                                   d_Tout, d_out, d_ng, d_st, stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    ng = d_ng.cpu().numpy().view(np.int32)
    Tout = d_Tout.cpu().numpy().view(np.float32).reshape(B, 16)
    st = d_st.cpu().numpy().reshape(B, STATS_BYTES) if stats else None
    return ng, Tout, d_out.cpu().numpy()[:total], st, off


def _batch_problems():
    """66 problems: every size near a per-thread or LDS boundary, fewer than 3 and fewer than 10 map points, empty, 8,192
    keypoints; mono, stereo and mixed."""
    probs = []
    seed = 500
    for n in (0, 2, 5, 9, 255, 256, 257, 1023, 1024, 1025, 8192):
        for sf in (0.0, 1.0, 0.5):
            p = ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=0.15, fill=1.0 if n < 10 else 0.85)
            if n > 1023:
                p["has_mp"][1023] = 1
            probs.append(p)
            seed += 1
    rng = np.random.default_rng(41)
    while len(probs) < 66:
        n = int(rng.choice([3, 10, 40, 60, 300, 700]))
        p = ps.make_problem(seed, n, stereo_frac=float(rng.uniform(0, 1)), outlier_frac=float(rng.uniform(0, 0.4)))
        if n == 40:
            p["has_mp"][:] = 0
            p["has_mp"][[4, 30]] = 1                      # 2 map points among 40 keypoints
        probs.append(p)
        seed += 1
    return probs


def test_device_batch_equals_host_batch_and_single_calls():
    probs = _batch_problems()
    assert len(probs) >= 64
    host = pose_optimization_batch(probs, ps.CAM, ps.inv_level_sigma2())
    ng, Tout, out, st, off = _device_batch(probs, stream=torch.cuda.Stream())
    for b, p in enumerate(probs):
        hm = p["has_mp"] > 0
        dev = (int(ng[b]), Tout[b], out[off[b]:off[b + 1]], st[b].tobytes())
        single = _dev(p)
        _same(dev, host[b], hm)
        _same(dev, single, hm)
        assert np.all(dev[2][~hm] == 0xAA)                 # never written where there is no map point
        if hm.sum() < 3:
            assert dev[0] == 0 and np.array_equal(dev[1], np.asarray(p["Tcw"], np.float32).reshape(16))
    # the null stream, and no stats: the same bits
    ng2, Tout2, out2, st2, _ = _device_batch(probs, stats=False)
    assert st2 is None and np.array_equal(ng2, ng) and np.array_equal(Tout2.view(np.uint32), Tout.view(np.uint32))
    assert np.array_equal(out2, out)


def test_device_batch_without_uright():
    """uright = NULL: every edge monocular, as the host forms' uright = NULL."""
    probs = [ps.make_problem(600 + i, n, stereo_frac=0.0, outlier_frac=0.2) for i, n in enumerate((0, 9, 257, 1025, 3000, 8192))]
    for p in probs:
        p["uright"] = None
    host = pose_optimization_batch(probs, ps.CAM, ps.inv_level_sigma2())
    ng, Tout, out, st, off = _device_batch(probs, uright=False, stream=torch.cuda.Stream())
    for b, p in enumerate(probs):
        _same((int(ng[b]), Tout[b], out[off[b]:off[b + 1]], st[b].tobytes()), host[b], p["has_mp"] > 0)


def test_device_batch_rejects_a_problem_alone():
    """More than 8,192 keypoints: ORBX_ERR_UNSUPPORTED.  A map point on a keypoint whose octave has no level (in the LDS-staged
    part or beyond it): ORBX_ERR_ARG.  Neither writes anything else; the problems around them come out as single calls do; an
    out-of-range octave where there is no map point is accepted, as the host forms accept it."""
    good = [ps.make_problem(700 + i, n, stereo_frac=0.5, outlier_frac=0.2) for i, n in enumerate((300, 1500, 50))]
    big = ps.make_problem(710, 8193, stereo_frac=0.5)
    lds_bad = ps.make_problem(711, 500, stereo_frac=0.5)
    lds_bad["has_mp"][3], lds_bad["octave"][3] = 1, -2
    far_bad = ps.make_problem(712, 2000, stereo_frac=0.5)
    far_bad["has_mp"][1500], far_bad["octave"][1500] = 1, 8           # nlevels = 8
    no_mp = ps.make_problem(713, 1200, stereo_frac=0.5, outlier_frac=0.1)
    no_mp["has_mp"][[10, 1100]] = 0
    no_mp["octave"][10], no_mp["octave"][1100] = -1, 40
    probs = [good[0], big, good[1], lds_bad, no_mp, far_bad, good[2]]
    ng, Tout, out, st, off = _device_batch(probs, stream=torch.cuda.Stream())
    for b, code in ((1, ERR_UNSUPPORTED), (3, ERR_ARG), (5, ERR_ARG)):
        assert ng[b] == code
        assert np.all(Tout[b].view(np.uint32) == 0xAAAAAAAA) and np.all(st[b] == 0xAA)
        assert np.all(out[off[b]:off[b + 1]] == 0xAA)
    for b in (0, 2, 4, 6):
        p = probs[b]
        hm = p["has_mp"] > 0
        _same((int(ng[b]), Tout[b], out[off[b]:off[b + 1]], st[b].tobytes()), _dev(p), hm)
        assert ng[b] > 0


# ------------------------------------------------------------------------------------------------ B. limits, against the restatement

BOUNDARY = [254, 255, 256, 1022, 1023, 1024]          # keypoints next to the per-thread and LDS boundaries always get a map point
LIMIT_SEEDS = {255: 302, 256: 303, 257: 302, 1023: 305, 1024: 300, 1025: 304, 8191: 301}


def _check(p):
    ref = po.run(p)
    _margins_ok(ref[3])
    assert ref[3].rounds == 4
    got = _dev(p)
    _agree(p, got, ref)
    return got


@pytest.mark.parametrize("n", sorted(LIMIT_SEEDS))
def test_sizes_at_the_thread_and_lds_boundaries(n):
    p = ps.make_problem(LIMIT_SEEDS[n], n, stereo_frac=0.5, outlier_frac=0.15)
    p["has_mp"][[i for i in BOUNDARY if i < n]] = 1
    _check(p)


def test_edges_only_beyond_the_lds_stage():
    """3,000 keypoints, map points only at indices >= 1024: every edge comes from the global-fetch path."""
    p = ps.make_problem(302, 3000, stereo_frac=0.5, outlier_frac=0.15)
    p["has_mp"][:1024] = 0
    got = _check(p)
    assert got[3].ninitial > 1500


@pytest.mark.parametrize("lane", [0, 255])
def test_edges_of_one_thread_only(lane):
    """8,192 keypoints, map points exactly at lane + 256 k: all 32 edges sit in one thread's mask bits 0 .. 31."""
    p = ps.make_problem(302, 8192, stereo_frac=1.0, outlier_frac=0.1, fill=0.0)
    p["has_mp"][lane::256] = 1
    got = _check(p)
    assert got[3].ninitial == 32


# (nlevels, scale, stereo fraction) -> seed.  Monocular scenes converge to the last bits within round 1, after which trials
# decide on rounding noise (tests/test_gpu_pose.py): they take 2 px of noise and the seeds with the widest rho margin.
LEVEL_SEEDS = {(6, 1.1, 0.0): 1071, (6, 1.1, 1.0): 303, (1, 1.2, 0.0): 1057, (1, 1.2, 1.0): 300, (32, 1.05, 0.0): 666,
               (32, 1.05, 1.0): 306}


@pytest.mark.parametrize("nlevels,scale,sf", sorted(LEVEL_SEEDS))
def test_pyramids(nlevels, scale, sf):
    """This fork's pyramid (6 levels at 1.1), a single level and the 32-level maximum (at 1.05), mono and stereo."""
    p = ps.make_problem(LEVEL_SEEDS[(nlevels, scale, sf)], 600, stereo_frac=sf, outlier_frac=0.15, nlevels=nlevels, scale=scale,
                        noise_px=0.5 if sf else 2.0)
    assert len(p["inv_sigma2"]) == nlevels and p["octave"].max() == nlevels - 1
    _check(p)


def test_uright_zero_and_negative_zero_are_stereo():
    """Optimizer.cc tests mvuRight[i] < 0: 0.0 and -0.0 both make stereo edges (here with a third error row far off)."""
    p = ps.make_problem(306, 400, stereo_frac=0.5, outlier_frac=0.1)
    st = np.flatnonzero((p["uright"] >= 0) & (p["has_mp"] > 0))
    p["uright"][st[:4]] = 0.0
    p["uright"][st[4:8]] = -0.0
    assert np.signbit(p["uright"][st[4:8]]).all()
    got = _check(p)
    assert got[2][st[:8]].all()                        # a stereo error of hundreds of pixels: outliers


def test_nan_map_point_returns_the_restatements_outputs():
    """A NaN coordinate in one map point: every sum of the normal equations is NaN, the LDLT finds no diagonal entry to pivot on
    and takes its zero-diagonal exit (x = 0), and every trial is rejected on a NaN chi2.  The restatement runs all four rounds to
    their limits, never flags the NaN edge (a NaN chi2 is not above its threshold) and flags the 11 others at the start pose, which
    no round leaves: the pose comes out as it went in, through one quaternion round trip.  The device must return the same
    outputs (the assertions of _agree; the margins are NaN here and are not checked).  Both behaviours of the LDLT's exit end in
    a rejected trial, so this pins the path's outputs, not the choice between them."""
    p = ps.make_problem(8, 12, stereo_frac=0.5, outlier_frac=0.0, fill=1.0)
    p["mp_pos"][0, 0] = np.nan
    ref = po.run(p)
    ng, T, out, st = ref
    assert ng == 1 and st.ninitial == 12 and st.rounds == 4
    assert list(st.iterations) == [10] * 4 and list(st.trials) == [10] * 4
    assert out[0] == 0 and out[1:].all()
    assert np.isfinite(T).all() and np.isfinite(list(st.q) + list(st.t)).all()
    assert _ulp_diff(T, p["Tcw"]).max() <= 1
    _agree(p, _dev(p), ref)


def _raw(p, form, frame=None, fill=0xAA):
    """One raw ctypes call with the outlier array pre-filled with `fill` (the Python wrappers zero it).  form: 'single',
    'frame' or 'batch' (host arrays).  Returns the outlier array."""
    L = lib()
    n = len(p["has_mp"])
    k = _kps(p["kp_xy"], p["octave"])
    ur = np.ascontiguousarray(p["uright"], np.float32)
    has = np.ascontiguousarray(p["has_mp"], np.uint8)
    mp = np.ascontiguousarray(p["mp_pos"], np.float32)
    cam = _camera(p["cam"], p["inv_sigma2"])
    Tin = np.ascontiguousarray(p["Tcw"], np.float32).reshape(16)
    Tout = np.zeros(16, np.float32)
    out = np.full(n, fill, np.uint8)
    ng = np.zeros(1, np.int32)
    vp = C.c_void_p
    a = lambda x: vp(x.ctypes.data)                    # noqa: E731
    if form == "single":
        rc = L.orbm_pose_optimization(a(k), a(ur), n, a(has), a(mp), C.byref(cam), a(Tin), a(Tout), a(out), a(ng), None)
    elif form == "frame":
        rc = L.orbm_frame_pose_optimization(frame._h, a(has), a(mp), C.byref(cam), a(Tin), a(Tout), a(out), a(ng), None)
    else:
        off = np.array([0, n], np.int32)
        rc = L.orbm_pose_optimization_batch(a(k), a(ur), a(off), 1, a(has), a(mp), C.byref(cam), a(Tin), a(Tout), a(out), a(ng), None, 0,
                                            None)
    assert rc == 0
    return out


def test_outlier_flags_kept_where_there_is_no_map_point():
    """mvbOutlier[i] is only written where mvpMapPoints[i] is set, in every form (host single, resident frame, host batch, device
    batch): 0xAA stays 0xAA elsewhere, and the flags written are those of the wrapper."""
    p = ps.make_problem(305, 1500, stereo_frac=0.5, outlier_frac=0.2, fill=0.6)
    hm = p["has_mp"] > 0
    ref = _dev(p)
    fr = Frame(_kps(p["kp_xy"], p["octave"]), np.zeros((1500, 32), np.uint8), (-1e4, -1e4, 1e4, 1e4), p["uright"])
    outs = [_raw(p, "single"), _raw(p, "frame", fr), _raw(p, "batch"), _device_batch([p])[2]]
    fr.close()
    for o in outs:
        assert np.all(o[~hm] == 0xAA)
        assert np.array_equal(o[hm], ref[2][hm])
    assert ref[2][hm].any()


# ------------------------------------------------------------------------------------------------ C. resident-frame and C++ forms

def test_frame_with_keypoints_outside_its_bounds():
    """Bounds that leave 10-30 % of the keypoints outside the grid (kept after the sorted part), map points on both kinds."""
    for seed, sf in ((320, 0.0), (321, 0.6)):
        p = ps.make_problem(seed, 2500, stereo_frac=sf, outlier_frac=0.2)
        bounds = (40.0, 30.0, 600.0, 450.0)
        x, y = p["kp_xy"][:, 0], p["kp_xy"][:, 1]
        inside = (x >= bounds[0]) & (x < bounds[2]) & (y >= bounds[1]) & (y < bounds[3])
        hm = p["has_mp"] > 0
        ur = p["uright"] if sf > 0 else None
        fr = Frame(_kps(p["kp_xy"], p["octave"]), np.zeros((2500, 32), np.uint8), bounds, ur)
        assert 0.1 * 2500 <= fr.n - fr.ns <= 0.3 * 2500
        assert (hm & ~inside).sum() > 100 and (hm & inside).sum() > 1024
        host = _dev(dict(p, uright=ur))
        res = _dev(p, frame=fr)
        fr.close()
        _same(res, host, np.ones(2500, bool))


def _backprojected_scene(kp_xy, octave, inv_sigma2, rng, stereo_frac=0.5):
    """Map points for keypoints at kp_xy: back-projected at random depths from a known pose, with 0.01 m noise and 20 % gross
    outliers; stereo right coordinates on a part of them.  Returns the problem dict of tests/pose_only_scene.py."""
    fx, fy, cx, cy, bf = ps.CAM
    n = len(octave)
    Rt, tt = ps.rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 0.5, 3)
    z = rng.uniform(1.0, 8.0, n)
    Pc = np.stack([(kp_xy[:, 0] - cx) / fx * z, (kp_xy[:, 1] - cy) / fy * z, z], 1)
    Xw = (Pc - tt) @ Rt + rng.normal(0, 0.01, (n, 3))
    bad = rng.random(n) < 0.2
    Xw[bad] += rng.normal(0, 0.5, (bad.sum(), 3))
    ur = np.where(rng.random(n) < stereo_frac, kp_xy[:, 0] - bf / z + rng.normal(0, 0.5, n), -1.0).astype(np.float32)
    R0 = ps.rodrigues(rng.normal(0, 0.03, 3)) @ Rt
    return {"kp_xy": kp_xy, "octave": octave, "uright": ur, "has_mp": (rng.random(n) < 0.9).astype(np.uint8),
            "mp_pos": Xw.astype(np.float32), "cam": np.array(ps.CAM, np.float32), "inv_sigma2": inv_sigma2,
            "Tcw": ps.pose44(R0, tt + rng.normal(0, 0.03, 3))}


def test_frame_from_the_extractor():
    """A frame from orbm_frame_from_extractor (this fork's 6-level, 1.1 pyramid) with undistorted coordinates and a host uright,
    against the host form fed the same undistorted coordinates."""
    ex = ORBextractor(1500, 1.1, 6, 20, 7)
    kps, desc = ex(synth_frame(3))
    n = len(kps)
    assert n > 1024
    rng = np.random.default_rng(330)
    xy = np.stack([kps["x"], kps["y"]], 1) + rng.uniform(-0.8, 0.8, (n, 2))
    xy = xy.astype(np.float32)
    inv = np.asarray(ex.GetInverseScaleSigmaSquares(), np.float32)
    p = _backprojected_scene(xy, kps["octave"].astype(np.int32), inv, rng)
    bounds = (0.0, 0.0, 640.0, 480.0)
    fr = Frame.from_extractor(ex, 0, bounds, xy_undistorted=xy, uright=p["uright"])
    res = _dev(p, frame=fr)
    fr.close()
    host = _dev(p)
    _same(res, host, np.ones(n, bool))
    assert host[0] > 0.6 * p["has_mp"].sum() and host[2][p["has_mp"] > 0].sum() > 0.1 * p["has_mp"].sum()


def test_cxx_class_both_overloads(tmp_path):
    """orbslam_hip::PoseOptimization's vector and frame-handle overloads (tests/cxx/pose_forms.cpp) on a stereo scene with
    keypoints outside the frame's bounds: the pose, flags and stats of the Python host form, bit for bit."""
    exe = tmp_path / "pose_forms"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "pose_forms.cpp"), SO_PATH, "-Wl,-rpath," + os.path.dirname(SO_PATH), "-o", str(exe)])
    p = ps.make_problem(340, 1800, stereo_frac=0.6, outlier_frac=0.2)
    n = len(p["has_mp"])
    bounds = np.array([30.0, 20.0, 620.0, 460.0], np.float32)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as f:
        f.write(np.array([n, len(p["inv_sigma2"]), 1], np.int32).tobytes())
        f.write(np.concatenate([p["cam"], p["inv_sigma2"], p["Tcw"].reshape(16), bounds]).astype(np.float32).tobytes())
        f.write(p["kp_xy"].astype(np.float32).tobytes() + p["octave"].astype(np.int32).tobytes())
        f.write(p["uright"].astype(np.float32).tobytes() + p["has_mp"].astype(np.uint8).tobytes())
        f.write(p["mp_pos"].astype(np.float32).tobytes())
    res = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(scene), str(res)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = res.read_bytes()
    one = 4 + 64 + n + STATS_BYTES
    assert len(data) == 2 * one
    host = _dev(p)
    for f in range(2):
        b = data[f * one:(f + 1) * one]
        got = (int(np.frombuffer(b[:4], np.int32)[0]), np.frombuffer(b[4:68], np.float32), np.frombuffer(b[68:68 + n], np.uint8),
               b[68 + n:])
        _same(got, (host[0], host[1].reshape(16), host[2], bytes(host[3])), np.ones(n, bool))


# ------------------------------------------------------------------------------------------------ D. independent checks of the optimum

@pytest.mark.parametrize("stereo", [False, True])
def test_noise_free_scene_on_the_device(stereo):
    """The true pose is the exact optimum (tests/pose_only_scene.py: noise_free): the device must land on it, with the bounds the
    restatement is held to in tests/test_cpu_pose_only.py."""
    p = ps.noise_free(1 + stereo, 200, stereo)
    ng, T, out, st = _dev(p)
    assert ng == 200 and not out.any() and st.rounds == 4
    q = np.array([0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)])          # Rt: 90 degrees about z
    assert np.abs(pm.quat_matrix(q) - p["Rt"]).max() < 1e-15
    assert np.abs(np.array(st.q) - q).max() < 1e-9
    assert np.abs(np.array(st.t) - p["tt"]).max() < (5e-9 if stereo else 1e-9)


@pytest.mark.parametrize("name", sorted(pm.SCENES))
def test_round_four_ends_at_the_optimum(name):
    """From the device's double pose, one float64 Gauss-Newton step on round 4's edges (the set round 3's classification left
    active, as the restatement reports it) is below STEP_TOL and gains less than GAIN_TOL of chi2.  The edge set is a discrete
    output: the device's classifications must be the restatement's (no chi2 near its threshold); the trial counts may differ
    where a trial decides on rounding noise, which moves the pose by far less than the tolerances."""
    seed, n, sf, of, kw = pm.SCENES[name]
    p = ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=of, **kw)
    ng, T, out, rst, edges = po.run(p, edges=True)
    assert rst.min_class > 1e-6
    assert rst.rounds == 4 and rst.iterations[3] < 10                   # round 4 stopped by Raul's criterion
    got = _dev(p)
    hm = p["has_mp"] > 0
    assert got[0] == ng and np.array_equal(got[2][hm], out[hm]) and got[3].rounds == 4
    assert got[3].iterations[3] < 10
    act = pm.round4_active(edges)
    step, gain, chi2 = pm.gauss_newton_check(p, act, got[3].q, got[3].t)
    assert step <= pm.STEP_TOL and gain <= pm.GAIN_TOL, (step, gain)
    assert chi2 > 0 and abs(chi2 - got[3].chi2) <= 1e-3 * chi2             # the cost is the one round 4 minimised
