"""The extractor chain on the device at content extremes: every scene of tests/extract_scenes.py (blurred pixels of exactly 0 and
255, row sums at both ends of 16 bits, the 257-tap clamp, angles of exactly 0 / 90 / 180 / 270, |m10| == |m01|, m10 == m01 == 0,
hundreds of candidates in one response class, contrasts either side of both FAST thresholds) against two yardsticks at once --
the numpy restatement (tests/extract_reference.py) and the C oracle -- through the stage getters, bit for bit.  Then the same
scenes as one batch of mixed content, under both forms of the pyramid / octree launches, in a batch long enough for the
256-thread k_octree, from rows with a pitch, and through one handle in turn.  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import extract_reference as ref
import extract_scenes as scenes
from orb_slam2_e_amd import ORBextractor

NAMES = [s.name for s in scenes.scenes()]
SAME_SIZE = [s.name for s in scenes.scenes() if s.image.shape == (scenes.H, scenes.W)]       # eleven frames of 200 x 260 (the lattice twice)
BATCH_PARAMS = scenes.LATTICE_PARAMS            # one handle for the mixed batches: the lattice keeps its quota of 60


@functools.lru_cache(maxsize=None)
def truth(name, params):
    """(restatement, oracle) of a scene under `params`: the scene's own come from the shared cache."""
    s = scenes.by_name(name)
    if params == s.params:
        r, o = scenes.restated(name), scenes.oracled(name)
    else:
        r, o = ref.run(s.image, params), scenes.oracle_run(s.image, params)
    for key in r.out:                           # the two yardsticks agree (tests/test_cpu_extract_reference.py holds them equal stage by stage)
        assert r.out[key][0].tobytes() == o.out[key][0].tobytes() and np.array_equal(r.out[key][1], o.out[key][1]), (name, key)
    return r, o


def _same_output(got, want, what):
    k, d = got
    wk, wd = want
    assert len(k) == len(wk), f"{what}: {len(k)} keypoints, expected {len(wk)}"
    for f in wk.dtype.names:
        assert k[f].tobytes() == wk[f].tobytes(), f"{what}: keypoint field {f}"
    assert np.array_equal(d, wd), f"{what}: descriptors"


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_against_both_yardsticks(name):
    s = scenes.by_name(name)
    r, o = truth(name, s.params)
    nlevels = s.params[2]
    for bv in (0, 1):
        ex = ORBextractor(*s.params, blur_variant=bv)
        got = ex(np.asarray(s.image))
        for l in range(nlevels):
            L = r.levels[l]
            if bv == 0:
                pad = ex.pyramid_level(0, l, padded=True)
                assert np.array_equal(pad, L.padded) and np.array_equal(pad, o.padded[l]), f"{name}: padded level {l}"
                c = ex.level_candidates(0, l)
                assert len(c) == len(L.cands) == len(o.cands[l]), f"{name}: level {l}: {len(c)} candidates, expected {len(L.cands)}"
                assert c.tobytes() == L.cands.tobytes(), f"{name}: candidates of level {l}"
                assert np.array_equal(c[:, 0], o.cands[l]["x"]) and np.array_equal(c[:, 1], o.cands[l]["y"]) and \
                    np.array_equal(c[:, 2], o.cands[l]["response"])
                k = ex.level_keypoints(0, l)
                assert len(k) == len(L.kps), f"{name}: level {l}: {len(k)} keypoints, expected {len(L.kps)}"
                assert k.tobytes() == L.kps.tobytes() == o.kps[l].tobytes(), f"{name}: keypoints of level {l} (angles as float bits)"
            b = ex.blurred_level(0, l)
            assert np.array_equal(b, r.blur[bv][l][0]) and np.array_equal(b, o.blurred[bv][l]), f"{name}: blurred level {l}, taps {bv}"
        _same_output(got, r.out[(bv, 0)], f"{name}, blur_variant {bv}")
        _same_output(got, o.out[(bv, 0)], f"{name}, blur_variant {bv} (oracle)")
    ex = ORBextractor(*s.params, trig_variant=1)
    got = ex(np.asarray(s.image))
    _same_output(got, r.out[(0, 1)], f"{name}, trig_variant 1")
    _same_output(got, o.out[(0, 1)], f"{name}, trig_variant 1 (oracle)")


def _batch_equals_truth(ex, names, what):
    kps, desc, cnt = ex.download_batch()
    for f, name in enumerate(names):
        r, _ = truth(name, BATCH_PARAMS)
        _same_output((kps[f, :cnt[f]], desc[f, :cnt[f]]), r.out[(0, 0)], f"{what}: frame {f} ({name})")


def test_one_batch_of_mixed_content():
    """All eleven 200 x 260 scenes as ONE batch: saturated, striped, tie-heavy and nearly empty frames side by side in every launch.
    Eleven frames are more than six, so k_octree runs its 256-thread form on the lattice's equal nodes here."""
    assert len(SAME_SIZE) == 11 and {"lattice", "binary_blocks", "stripes", "symmetric_marks"} <= set(SAME_SIZE)
    frames = np.stack([scenes.by_name(n).image for n in SAME_SIZE])
    ex = ORBextractor(*BATCH_PARAMS)
    ex.extract_batch(frames)
    _batch_equals_truth(ex, SAME_SIZE, "batch of eleven")
    for f, name in enumerate(SAME_SIZE):
        r, _ = truth(name, BATCH_PARAMS)
        _same_output(ex.download(f), r.out[(0, 0)], f"download({f}) ({name})")
        for l in range(BATCH_PARAMS[2]):
            assert np.array_equal(ex.pyramid_level(f, l, padded=True), r.levels[l].padded), (name, l)
            assert np.array_equal(ex.blurred_level(f, l), r.blur[0][l][0]), (name, l)
            assert ex.level_candidates(f, l).tobytes() == r.levels[l].cands.tobytes(), (name, l)
            assert ex.level_keypoints(f, l).tobytes() == r.levels[l].kps.tobytes(), (name, l)


@pytest.mark.parametrize("limit", ["64", "0"])
def test_both_forms_of_the_pyramid_and_octree_launches(limit, monkeypatch):
    """ORBX_PYR_CHAIN_MAX_BATCH / ORBX_OCT_WIDE_MAX_BATCH (read per call): levels 1.. in one launch with the 512-thread k_octree, or a
    launch per level with the 256-thread one -- one frame, a batch of three and the batch of eleven under each."""
    monkeypatch.setenv("ORBX_PYR_CHAIN_MAX_BATCH", limit)
    monkeypatch.setenv("ORBX_OCT_WIDE_MAX_BATCH", limit)
    ex = ORBextractor(*BATCH_PARAMS)
    for name in ("lattice", "binary_blocks", "stripes"):
        r, _ = truth(name, BATCH_PARAMS)
        _same_output(ex(np.asarray(scenes.by_name(name).image)), r.out[(0, 0)], f"limit {limit}: {name}")
        for l in range(BATCH_PARAMS[2]):
            assert np.array_equal(ex.pyramid_level(0, l, padded=True), r.levels[l].padded), (limit, name, l)
            assert ex.level_keypoints(0, l).tobytes() == r.levels[l].kps.tobytes(), (limit, name, l)
    three = ["lattice", "checker8", "threshold_edges_255"]
    ex.extract_batch(np.stack([scenes.by_name(n).image for n in three]))
    _batch_equals_truth(ex, three, f"limit {limit}: batch of three")
    ex.extract_batch(np.stack([scenes.by_name(n).image for n in SAME_SIZE]))
    _batch_equals_truth(ex, SAME_SIZE, f"limit {limit}: batch of eleven")


@pytest.mark.parametrize("pad", [4, 13])
def test_rows_with_a_pitch_larger_than_the_width(pad):
    """Every scene from rows `width + pad` bytes apart (a dword-aligned pitch and one that is not); the bytes between the rows are
    poisoned with a value no scene of 0 / 255 content would hide, and the buffer ends with the last pixel."""
    from orb_slam2_e_amd._lib import check
    from orb_slam2_e_amd.extractor import KP_DTYPE
    for name in NAMES:
        s = scenes.by_name(name)
        r, _ = truth(name, s.params)
        h, w = s.image.shape
        stride = w + pad
        buf = np.full((h - 1) * stride + w, 0xA5, np.uint8)
        for y in range(h):
            buf[y * stride: y * stride + w] = s.image[y]
        ex = ORBextractor(*s.params)
        ex._reserve(w, h, 1)
        kps = np.zeros(ex.capacity, KP_DTYPE); desc = np.zeros((ex.capacity, 32), np.uint8); n = C.c_int(0)
        check(ex._L.orbx_extract(ex._h, buf.ctypes.data_as(C.c_void_p), w, h, stride, kps.ctypes.data_as(C.c_void_p),
                                 desc.ctypes.data_as(C.c_void_p), ex.capacity, C.byref(n)))
        _same_output((kps[:n.value], desc[:n.value]), r.out[(0, 0)], f"{name}, pitch {stride}")


def test_one_handle_serves_the_scenes_in_turn():
    """One handle, the cached plan: a tie-heavy frame after a saturated one, an empty-ish one after that, then the batch and a
    single frame again -- every result the same as a fresh handle gives against the yardsticks."""
    ex = ORBextractor(*BATCH_PARAMS)
    order = ["binary_blocks", "lattice", "threshold_edges_0", "checker8", "lattice", "stripes", "symmetric_marks", "threshold_edges_255",
             "binary_blocks", "lattice"]
    for step, name in enumerate(order):
        r, _ = truth(name, BATCH_PARAMS)
        _same_output(ex(np.asarray(scenes.by_name(name).image)), r.out[(0, 0)], f"step {step}: {name}")
        for l in range(BATCH_PARAMS[2]):
            assert ex.level_keypoints(0, l).tobytes() == r.levels[l].kps.tobytes(), (step, name, l)
    ex.extract_batch(np.stack([scenes.by_name(n).image for n in SAME_SIZE]))
    _batch_equals_truth(ex, SAME_SIZE, "batch after single frames")
    r, _ = truth("lattice", BATCH_PARAMS)
    _same_output(ex(np.asarray(scenes.by_name("lattice").image)), r.out[(0, 0)], "lattice after the batch")
    # another size through the same handle (a new plan), and back
    for name in ("odd_sizes", "lattice", "odd_sizes"):
        r, _ = truth(name, BATCH_PARAMS)
        _same_output(ex(np.asarray(scenes.by_name(name).image)), r.out[(0, 0)], f"{name} after a change of size")
