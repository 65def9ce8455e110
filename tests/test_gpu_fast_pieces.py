"""k_fast_cells' tile load in 16-byte pieces, on the device, at the geometries where it can go wrong: the narrowest and the widest
cell of each of the three tile-row variants (52, 64 and 80 bytes: cells of 30 / 44, 45 / 52 and 53 / 59 px), cells taller than one
chunk of load instructions (48 rows), the frame whose last cell of the last level reads as close to the end of its padded row as
the cell grid allows, that frame from rows with a pitch inside a poisoned parent, batches of 7 and of 8 distinct frames (the two
forms of the workgroup-to-frame mapping), and cells that are empty at iniThFAST beside cells that are not.  Every stage against
the numpy restatement and the C oracle, bit for bit, as tests/test_gpu_extract_content.py does."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import extract_reference as ref
import extract_scenes as scenes
from orb_slam2_e_amd import ORBextractor
from orb_slam2_e_amd.extractor import FAST_PIECE_FIELDS, fast_pieces, plan

COL = {n: i for i, n in enumerate(FAST_PIECE_FIELDS)}
ONE = (300, 1.2, 1, 20, 7)
REACH = (300, 1.2, 3, 20, 7)
REACH_HW = (103, 110)          # the last cell of level 2 ends 20 bytes before the end of the border: the least the grid allows
# name: (h, w, params, tile stride, widest cell, tallest cell)
GEOMS = {
    "ts52_cw30": (62, 62, ONE, 52, 30, 30),
    "ts52_cw44": (75, 76, ONE, 52, 44, 43),
    "ts52_two_chunks": (91, 76, ONE, 52, 44, 59),
    "ts64_cw45": (75, 77, ONE, 64, 45, 43),
    "ts64_cw52": (75, 84, ONE, 64, 52, 43),
    "ts80_cw53": (75, 85, ONE, 80, 53, 43),
    "ts80_cw59_two_chunks": (91, 91, ONE, 80, 59, 59),
    "reach": REACH_HW + (REACH, 64, 45, 54),
}


def image(h, w, seed):
    """noise (a corner candidate in most 4-pixel groups) on the right, the scenes' mixed content on the left"""
    img = scenes.mixed(h, w, seed)[0].copy()
    img[:, w // 2:] = np.random.default_rng(seed).integers(0, 256, (h, w - w // 2), dtype=np.uint8)
    img.flags.writeable = False
    return img


@functools.lru_cache(maxsize=None)
def truth(h, w, seed, params, oracle=True):
    img = image(h, w, seed)
    r = ref.run(img, params)
    o = scenes.oracle_run(img, params) if oracle else None
    return img, r, o


def _same_output(got, want, what):
    k, d = got
    wk, wd = want
    assert len(k) == len(wk), f"{what}: {len(k)} keypoints, expected {len(wk)}"
    for f in wk.dtype.names:
        assert k[f].tobytes() == wk[f].tobytes(), f"{what}: keypoint field {f}"
    assert np.array_equal(d, wd), f"{what}: descriptors"


def _stages(ex, frame, r, o, nlevels, what):
    for l in range(nlevels):
        L = r.levels[l]
        pad = ex.pyramid_level(frame, l, padded=True)
        assert np.array_equal(pad, L.padded) and (o is None or np.array_equal(pad, o.padded[l])), f"{what}: padded level {l}"
        c = ex.level_candidates(frame, l)
        assert len(c) == len(L.cands), f"{what}: level {l}: {len(c)} candidates, expected {len(L.cands)}"
        assert c.tobytes() == L.cands.tobytes(), f"{what}: candidates of level {l}"
        k = ex.level_keypoints(frame, l)
        assert k.tobytes() == L.kps.tobytes(), f"{what}: keypoints of level {l}"
        if o is not None:
            assert np.array_equal(c[:, 0], o.cands[l]["x"]) and np.array_equal(c[:, 1], o.cands[l]["y"]) and \
                np.array_equal(c[:, 2], o.cands[l]["response"]), f"{what}: candidates of level {l} (oracle)"
            assert k.tobytes() == o.kps[l].tobytes(), f"{what}: keypoints of level {l} (oracle)"


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_tile_variants_and_cell_sizes(name):
    h, w, params, ts, cw, ch = GEOMS[name]
    cells = fast_pieces(*params, w, h)
    assert plan(*params, w, h)["fast_tile_stride"] == ts and cells[:, COL["cw"]].max() == cw and cells[:, COL["rows"]].max() == ch
    img, r, o = truth(h, w, 3, params)
    assert sum(len(L.cands) for L in r.levels) > 20
    ex = ORBextractor(*params)
    got = ex(np.asarray(img))
    _stages(ex, 0, r, o, params[2], name)
    _same_output(got, r.out[(0, 0)], name)
    _same_output(got, o.out[(0, 0)], name + " (oracle)")


def test_the_reach_frame_from_a_pitched_region_of_interest():
    """The frame as a view into a larger parent full of a value the frame does not favour: rows 141 bytes apart, first pixel at an
    odd address.  The last cell of the last level is the one whose last piece ends nearest to the end of its row."""
    h, w = REACH_HW
    cells = fast_pieces(*REACH, w, h)
    info = plan(*REACH, w, h)
    last = cells[-1]
    assert last[COL["level"]] == 2
    stride = last[COL["stride"]]
    end = last[COL["img_off"]] % stride + 16 * last[COL["pieces"]]         # (levels start at multiples of 256 and strides are multiples of 64)
    assert 32 + info["level_w"][2] + 19 - end == 20
    img, r, o = truth(h, w, 3, REACH)
    parent = np.full((h + 9, w + 31), 0xA5, np.uint8)
    view = parent[4:4 + h, 13:13 + w]
    view[:] = img
    ex = ORBextractor(*REACH)
    got = ex(view)
    _stages(ex, 0, r, o, 3, "pitched")
    _same_output(got, r.out[(0, 0)], "pitched")
    _same_output(got, o.out[(0, 0)], "pitched (oracle)")


@pytest.mark.parametrize("batch", [7, 8])
def test_batches_of_seven_and_eight_distinct_frames(batch):
    """Eight frames go to the XCDs frame by frame (xcd_frame_item), seven do not; the last frame's last cell is the last thing
    the pyramid allocation holds."""
    h, w = REACH_HW
    frames = np.stack([image(h, w, 10 + f) for f in range(batch)])
    ex = ORBextractor(*REACH)
    ex.extract_batch(frames)
    kps, desc, cnt = ex.download_batch()
    for f in range(batch):
        _, r, o = truth(h, w, 10 + f, REACH, oracle=(f == batch - 1))
        _stages(ex, f, r, o, 3, f"batch of {batch}: frame {f}")
        _same_output((kps[f, :cnt[f]], desc[f, :cnt[f]]), r.out[(0, 0)], f"batch of {batch}: frame {f}")
        if o is not None:
            _same_output((kps[f, :cnt[f]], desc[f, :cnt[f]]), o.out[(0, 0)], f"batch of {batch}: frame {f} (oracle)")


def test_cells_empty_at_the_first_threshold_beside_cells_that_are_not():
    """Left: noise.  Right: single pixels of contrast 12 on a flat ground -- corners at minThFAST = 7 only, so those cells run the
    second pass while their neighbours in the same launch do not."""
    h, w = 75, 140
    img = np.full((h, w), 100, np.uint8)
    img[:, :60] = np.random.default_rng(4).integers(0, 256, (h, 60), dtype=np.uint8)
    img[6::9, 66::9] = 112
    r = ref.run(img, ONE)
    o = scenes.oracle_run(img, ONE)
    c = r.levels[0].cands
    weak = c[c[:, 0] > 60]
    assert len(weak) > 10 and weak[:, 2].max() < 20 and c[:, 2].max() >= 20, "the scene does not reach the second pass"
    ex = ORBextractor(*ONE)
    got = ex(img)
    _stages(ex, 0, r, o, 1, "second pass")
    _same_output(got, r.out[(0, 0)], "second pass")
    _same_output(got, o.out[(0, 0)], "second pass (oracle)")
