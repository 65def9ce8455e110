"""The whole-map relocalisation search under P poses in one launch (orbm_search_by_projection_map_poses,
orbm_frame_search_by_projection_map_poses on an orbm_map snapshot; k_map_search_poses): every row equals the oracle's and the
single-pose search's for that pose, does not depend on the other poses of the call, and is the same through every form.
Scenes: tests/map_poses_scenes.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from map_poses_scenes import CAP_SCENE, SCENES, oracle_pose, oracle_rows, scene
from orb_slam2_e_amd import Frame, MapSnapshot, ORBmatcher, OrbxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
ALL = SCENES + [CAP_SCENE]
M = ORBmatcher(0.6)
_handles = {}


def handles(sc):
    """(scene, resident frame, snapshot): made once per scene and shared"""
    if sc not in _handles:
        s = scene(*sc)
        _handles[sc] = (s, Frame(s["kps"], s["desc"], (0.0, 0.0, 640.0, 480.0)), MapSnapshot(s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"]))
    return _handles[sc]


def search(sc, poses=None, has_mp=None, want_proj=True):
    s, F, snap = handles(sc)
    poses = range(sc[3]) if poses is None else poses
    return M.frame_search_by_projection_map_poses(F, s["has_mp"] if has_mp is None else has_mp, snap, s["Rcw"][list(poses)], s["tcw"][list(poses)],
                                                  s["cam"], s["sf"], s["th"], want_proj)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("sc", ALL)
def test_every_row_equals_the_oracle(sc):
    got = search(sc)
    ref = oracle_rows(*sc)
    assert got[2].shape == ref[2].shape == (sc[3], sc[1], 4)
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))      # u, v, viewCos, level: float bits
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    assert ORBmatcher.last_map_poses_waits() == 1                               # a launched call waited once


@pytest.mark.parametrize("sc", ALL)
def test_every_row_equals_the_single_pose_search(sc):
    s, F, _ = handles(sc)
    got = search(sc)
    for p in range(sc[3]):
        one = M.frame_search_by_projection_map(F, s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], s["Rcw"][p], s["tcw"][p],
                                               s["cam"], s["sf"], s["th"])
        assert np.array_equal(got[0][p], one[0]) and got[1][p] == one[1]
        assert np.array_equal(got[2][p].view(np.uint32), one[2].view(np.uint32))


@pytest.mark.parametrize("sc", ALL)
def test_a_pose_does_not_depend_on_its_batch(sc):
    P = sc[3]
    full = search(sc)
    assert same(full, search(sc))                                               # a second run
    back = search(sc, range(P - 1, -1, -1))                                     # every pose at another place
    assert same(full, tuple(a[::-1] for a in back))
    for p in range(P):                                                          # alone
        alone = search(sc, [p])
        assert same(tuple(a[p:p + 1] for a in full), alone)
    q = P - 2 if P > 2 else P - 1
    twice = search(sc, [q, 0, q])                                               # listed twice: both rows, and equal to the row in the batch
    for r in (0, 2):
        assert same(tuple(a[r:r + 1] for a in twice), tuple(a[q:q + 1] for a in full))


@pytest.fixture(scope="module")
def forms_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_poses") / "map_poses_forms")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "map_poses_forms.cpp"),
                           "-o", exe, "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_scene(path, s, P):
    with open(path, "wb") as f:
        f.write(struct.pack("<4if", len(s["kps"]), len(s["pos"]), P, len(s["sf"]), s["th"]))
        for a in (s["cam"], s["kps"], s["desc"], s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"],
                  s["Rcw"][:P].astype(np.float64), s["tcw"][:P].astype(np.float64), s["sf"]):
            f.write(np.ascontiguousarray(a).tobytes())


@pytest.mark.parametrize("sc", [SCENES[2], SCENES[3]])
def test_host_arrays_snapshot_and_cxx_class_give_the_same_bytes(sc, forms_exe, tmp_path):
    s, _, _ = handles(sc)
    n, P = sc[2], sc[3]
    res = search(sc)
    host = M.SearchByProjectionMapPoses(s["kps"], s["desc"], s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], s["Rcw"], s["tcw"],
                                        s["cam"], s["sf"], s["th"])
    assert same(res, host)
    write_scene(tmp_path / "scene.bin", s, P)
    out = subprocess.run([forms_exe, str(tmp_path / "scene.bin"), str(tmp_path / "rows.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    rows = np.fromfile(tmp_path / "rows.bin", np.int32).reshape(2, P * n + P)
    for form in rows:                                                           # ResidentFrame form, FrameView form
        assert form[:P * n].tobytes() == res[0].tobytes() and form[P * n:].tobytes() == res[1].tobytes()


def test_one_snapshot_serves_other_masks_poses_and_frames():
    sc = SCENES[3]
    s, F, snap = handles(sc)
    full = search(sc)
    nop = search(sc, want_proj=False)                                           # proj = NULL is accepted
    assert nop[2] is None and np.array_equal(nop[0], full[0]) and np.array_equal(nop[1], full[1])
    free = np.zeros(sc[2], np.uint8)                                            # another mask, other poses, the same snapshot
    got = search(sc, [3, 1], free)
    for r, p in enumerate((3, 1)):
        ref = oracle_pose(s, p, has_mp=free)
        assert np.array_equal(got[0][r], ref[0]) and got[1][r] == ref[1] and np.array_equal(got[2][r].view(np.uint32), ref[2].view(np.uint32))
    assert not np.array_equal(got[0][1], full[0][1])                            # (the mask matters in this scene)
    none = M.frame_search_by_projection_map_poses(F, None, snap, s["Rcw"][[3, 1]], s["tcw"][[3, 1]], s["cam"], s["sf"], s["th"])
    assert same(none, got)                                                      # has_mappoint = NULL: no keypoint holds a point
    half = sc[2] // 2                                                           # a second frame on the same snapshot
    F2 = Frame(s["kps"][:half], s["desc"][:half], (0.0, 0.0, 640.0, 480.0))
    got2 = M.frame_search_by_projection_map_poses(F2, s["has_mp"][:half], snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])
    for p in range(sc[3]):
        ref = oracle_pose(s, p, has_mp=s["has_mp"][:half], kps=s["kps"][:half], desc=s["desc"][:half])
        assert np.array_equal(got2[0][p], ref[0]) and got2[1][p] == ref[1]
    assert same(full, search(sc))                                               # and the first frame's rows are what they were
    F2.close()


def test_every_keypoint_taken_gives_no_match_but_projections():
    sc = SCENES[2]
    got = search(sc, has_mp=np.ones(sc[2], np.uint8))
    assert (got[0] == -1).all() and (got[1] == 0).all()
    assert np.array_equal(got[2].view(np.uint32), oracle_rows(*sc)[2].view(np.uint32)) and (got[2][0, :, 3] >= 0).sum() > sc[1] // 4


def test_keypoints_outside_the_grid():
    sc = SCENES[2]
    s, _, snap = handles(sc)
    kps = s["kps"].copy()
    kps["x"][::7] = -30.0; kps["y"][3::11] = 500.0; kps["x"][5::13] = 640.0    # left of, below and on the far edge of the grid (cell 64 of 0 .. 63)
    F = Frame(kps, s["desc"], (0.0, 0.0, 640.0, 480.0))
    assert F.ns < F.n
    got = M.frame_search_by_projection_map_poses(F, s["has_mp"], snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])
    host = M.SearchByProjectionMapPoses(kps, s["desc"], s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], s["Rcw"], s["tcw"],
                                        s["cam"], s["sf"], s["th"])
    assert same(got, host)
    for p in range(sc[3]):
        ref = oracle_pose(s, p, kps=kps)
        assert np.array_equal(got[0][p], ref[0]) and got[1][p] == ref[1]
    out = np.zeros(sc[2], bool); out[::7] = True; out[3::11] = True; out[5::13] = True
    assert F.n - F.ns >= out.sum()                                              # (some clutter already lies on the far edge)
    assert (got[0][:, out] == -1).all() and got[1].sum() > 0
    F.close()


def test_nothing_to_search_launches_nothing():
    sc = SCENES[0]
    s, F, snap = handles(sc)
    search(sc)
    assert ORBmatcher.last_map_poses_waits() == 1
    empty_map = MapSnapshot(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 32), np.uint8))
    assert empty_map.m == 0
    got = M.frame_search_by_projection_map_poses(F, s["has_mp"], empty_map, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])     # m = 0
    assert ORBmatcher.last_map_poses_waits() == 0 and got[0].shape == (2, sc[2]) and (got[0] == -1).all() and (got[1] == 0).all() and got[2].shape == (2, 0, 4)
    search(sc)
    empty_frame = Frame(s["kps"][:0], s["desc"][:0], (0.0, 0.0, 640.0, 480.0))
    got = M.frame_search_by_projection_map_poses(empty_frame, None, snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])         # n = 0
    assert ORBmatcher.last_map_poses_waits() == 0 and got[0].shape == (2, 0) and (got[1] == 0).all()
    search(sc)
    got = search(sc, [])                                                                                                          # P = 0
    assert ORBmatcher.last_map_poses_waits() == 0 and got[0].shape == (0, sc[2]) and got[1].shape == (0,)
    search(sc)
    got = M.SearchByProjectionMapPoses(s["kps"], s["desc"], s["has_mp"], s["pos"][:0], s["nrm"][:0], s["mind"][:0], s["maxd"][:0], s["mp_desc"][:0],
                                       s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])                                           # host arrays, m = 0
    assert ORBmatcher.last_map_poses_waits() == 0 and (got[0] == -1).all() and (got[1] == 0).all()


def test_more_than_sixteen_poses_are_refused():
    sc = CAP_SCENE
    s, F, snap = handles(sc)
    R = np.concatenate([s["Rcw"], s["Rcw"][:1]]); t = np.concatenate([s["tcw"], s["tcw"][:1]])
    with pytest.raises(OrbxError) as e:
        M.frame_search_by_projection_map_poses(F, s["has_mp"], snap, R, t, s["cam"], s["sf"], s["th"])
    assert e.value.code == -5                                                   # ORBX_ERR_UNSUPPORTED
    with pytest.raises(OrbxError) as e:
        M.SearchByProjectionMapPoses(s["kps"], s["desc"], s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], R, t, s["cam"], s["sf"],
                                     s["th"])
    assert e.value.code == -5
    assert same(search(sc), oracle_rows(*sc))                                   # sixteen are served
