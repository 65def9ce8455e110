"""k_pyr_resize resamples the image rows once and copies the REFLECT_101 border from registers (rows: a second store; columns: bytes
of the neighbouring lanes' dwords).  Every padded level -- border and interior -- must stay what it was, byte for byte:
  * the per-level launches against the oracle's padded levels and against the one-launch chain (ORBX_PYR_CHAIN_MAX_BATCH is read per call),
  * keypoints and descriptors against oracle.OrbOracle.extract,
at the smallest frames that reach every way the kernel cuts a row into waves.

A padded row's dwords (3 .. xhi) are cut from the left into full waves of 64; what is left over goes to a tile of the row's last
16, 32 or 64 dwords x 4, 2 or 1 row groups, which also takes the right border where the last full wave reaches into it.  What can go
wrong depends on w mod 4 (the dword that straddles the right image edge), on the number of full waves (0: both borders in the tile;
1; 2 and more: waves without a border), on the tile's width and on a leftover at its limits (1, 16, 17, 32, 33, 63 dwords; none: the
last full wave holds the border), and on the last full wave reaching into the border, at every w mod 4.  The widths below reach all of
them at some level, and also the level widths whose group count is 1, 2 or 63 mod 64 (a last wave of 1, 2, 63 groups in a cut that
counts 64 groups from pixel 0).  test_the_widths_reach_every_cut checks that on the CPU, so that a change of the level rounding cannot
quietly empty the set.

orbx_reserve refuses a frame with a level under 62 px on a side (the 30-px FAST cell grid), so a level narrower or lower than 20 px --
where the copy rule does not hold and k_pyr_resize_small serves -- cannot be reached through the API: test_no_level_under_twenty_pixels
pins that down.  The smallest levels that can be reached (62 rows: border rows 1..19 and h-20..h-2 in row groups 0-2 and 5-7) are here,
and so is a level whose scale breaks the 8-byte-window rule, which does select k_pyr_resize_small."""
import ctypes as C

import numpy as np
import pytest

import oracle
from orb_slam2_e_amd import ORBextractor
from orb_slam2_e_amd.extractor import KP_DTYPE, plan
from orb_slam2_e_amd.synth import synth_frame

FOUR = (300, 1.2, 4, 20, 7)         # three resized levels: small frames still pass the cell-grid limit at the top
FORK = (1200, 1.1, 6, 24, 7)        # the fork's launch files
WIDTHS = (257, 258, 259, 260, 512, 516, 314, 302, 333, 410, 571, 108, 265, 308)
HEIGHT = 107                        # levels of 89, 74 and 62 rows: none a multiple of 8, the last the lowest the planner accepts


def _cut(w):
    """(full waves, tile width as a shift or 0, leftover dwords, the last full wave reaches into the right border) of a level of width w"""
    xlo, xhi = 3, (32 + w + 18) >> 2
    ndw = xhi - xlo + 1
    nfull, rem = divmod(ndw, 64)
    tws = 0 if rem == 0 else 4 if rem <= 16 else 5 if rem <= 32 else 6
    return nfull, tws, rem, rem != 0 and 8 + (w >> 2) < xlo + 64 * nfull


def test_the_widths_reach_every_cut():
    seen = {k: set() for k in ("nfull", "tws", "rem", "reach", "groups", "w4")}
    heights = set()
    for w in WIDTHS:
        p = plan(*FOUR, w, HEIGHT)
        for l in range(1, p["nlevels"]):
            wl = p["level_w"][l]
            nfull, tws, rem, reach = _cut(wl)
            seen["nfull"].add(min(nfull, 2)); seen["tws"].add(tws); seen["rem"].add(rem); seen["groups"].add(((wl + 3) // 4) % 64); seen["w4"].add(wl % 4)
            if reach:
                seen["reach"].add(wl % 4)
            heights.add(p["level_h"][l])
    assert seen["nfull"] == {0, 1, 2} and seen["tws"] == {0, 4, 5, 6} and seen["w4"] == {0, 1, 2, 3} and seen["reach"] == {0, 1, 2, 3}
    assert {1, 16, 17, 32, 33, 63} <= seen["rem"] and {1, 2, 63} <= seen["groups"]
    assert all(h % 8 for h in heights) and min(heights) == 62
    assert _cut(plan(500, 1.2, 8, 20, 7, 1242, 375)["level_w"][1])[0] == 4      # test_heights_and_scales: waves between the edge waves


def test_no_level_under_twenty_pixels():
    """The planner refuses what would give a level under 62 px a side, whichever the settings: no pyramid has a level the copy
    rule's single mirror fold (w, h >= 20) does not cover."""
    for prm, (w, h) in ((FORK, (40, 30)), (FORK, (31, 64)), (FORK, (99, 120)), (FOUR, (106, 105)), ((300, 1.2, 8, 20, 7), (70, 70))):
        with pytest.raises(Exception):
            plan(*prm, w, h)
    p = plan(*FOUR, 107, 107)
    assert min(p["level_w"]) == 62 and min(p["level_h"]) == 62


def _frames(n, h, w, seed):
    """n different images (another scene each, plus noise: a flat border region would hide a shifted byte)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        f = synth_frame(seed + k, max(w, 64), max(h, 64))[:h, :w]
        out.append(np.ascontiguousarray(np.clip(f.astype(np.int16) + rng.integers(-9, 10, f.shape), 0, 255).astype(np.uint8)))
    return out


def _reference(frames, params):
    o = oracle.OrbOracle(*params)
    ref = []
    for img in frames:
        kps, desc = o.extract(img)
        levels = []
        for l in range(params[2]):
            w, _, _ = o.level_dims(l)
            levels.append(o.level_padded(l)[:, :w + 38])
        ref.append((kps, desc, levels))
    return ref


def _same_keypoints(a, b):
    assert len(a) == len(b)
    for f in a.dtype.names:
        x, y = (a[f].view(np.uint32), b[f].view(np.uint32)) if a[f].dtype.kind == "f" else (a[f], b[f])
        assert np.array_equal(x, y), f"field {f} differs"


def _check_both_forms(frames, params, monkeypatch, ref=None):
    ref = ref or _reference(frames, params)
    for form, limit in (("levels", "0"), ("chain", "64")):
        monkeypatch.setenv("ORBX_PYR_CHAIN_MAX_BATCH", limit)
        ex = ORBextractor(*params)
        if len(frames) == 1:
            got = [ex(frames[0])]
        else:
            ex.extract_batch(np.stack(frames))
            kb, db, cb = ex.download_batch()
            got = [(kb[f, :cb[f]], db[f, :cb[f]]) for f in range(len(frames))]
        for f, (okps, odesc, olevels) in enumerate(ref):
            for l in range(params[2]):
                lev = ex.pyramid_level(f, l, padded=True)
                assert lev.shape == olevels[l].shape
                bad = np.argwhere(lev != olevels[l])
                assert len(bad) == 0, f"{form}: frame {f} level {l} ({lev.shape[1] - 38} x {lev.shape[0] - 38}): {len(bad)} bytes differ, first at padded (row, col) {tuple(bad[0])}"
            _same_keypoints(got[f][0], okps)
            assert np.array_equal(got[f][1], odesc), f"{form}: frame {f} descriptors differ"


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_every_cut_of_a_row(width, monkeypatch):
    _check_both_forms(_frames(1, HEIGHT, width, width), FOUR, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,params", [
    ((110, 257), FOUR),                      # 92, 76, 64 rows: a last row group that is full
    ((100, 101), FORK),                      # the fork's six levels on the smallest frame they accept: 63 x 62 at the top
    ((130, 250), (300, 2.0, 2, 20, 7)),      # scale 2: a group's source columns fill the 8-byte window exactly; 125 x 65
    ((375, 1242), (500, 1.2, 8, 20, 7)),     # KITTI: four full waves and a tile across level 1
])
def test_heights_and_scales(shape, params, monkeypatch):
    _check_both_forms(_frames(1, shape[0], shape[1], 3), params, monkeypatch)


@pytest.mark.gpu
def test_a_scale_that_breaks_the_window_rule(monkeypatch):
    """Scale 2.5: four output pixels take their sources from 9-10 columns, no 8-byte window holds them, and the level goes through
    k_pyr_resize_small (no chain either: both settings run the same kernel) -- the padded level still equals the oracle's."""
    _check_both_forms(_frames(2, 160, 200, 11), (300, 2.5, 2, 20, 7), monkeypatch)


@pytest.mark.gpu
def test_a_batch_of_seven_different_frames(monkeypatch):
    """Seven frames is the first batch that takes the per-level launches by default (and a grid whose frame count is no multiple of 8);
    with 64 as the limit the same batch goes through the chain.  Every frame is another image: bytes fetched from a neighbouring
    frame would show."""
    frames = _frames(7, HEIGHT, 313, 21)
    assert len({f.tobytes() for f in frames}) == 7
    monkeypatch.delenv("ORBX_PYR_CHAIN_MAX_BATCH", raising=False)
    ex = ORBextractor(*FOUR)
    ex.extract_batch(np.stack(frames))
    default = [ex.pyramid_level(f, l, padded=True) for f in range(7) for l in range(4)]
    ref = _reference(frames, FOUR)
    _check_both_forms(frames, FOUR, monkeypatch, ref)
    for f in range(7):
        for l in range(4):
            assert np.array_equal(default[f * 4 + l], ref[f][2][l])


@pytest.mark.gpu
def test_a_batch_of_eight_takes_whole_frames_per_xcd(monkeypatch):
    """A frame count that is a multiple of 8 switches the (frame, item) mapping of the grid; different images again."""
    monkeypatch.setenv("ORBX_PYR_CHAIN_MAX_BATCH", "0")
    frames = _frames(8, HEIGHT, 299, 40)
    ref = _reference(frames, FOUR)
    ex = ORBextractor(*FOUR)
    ex.extract_batch(np.stack(frames))
    for f in range(8):
        for l in range(4):
            assert np.array_equal(ex.pyramid_level(f, l, padded=True), ref[f][2][l]), (f, l)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [4, 13])
def test_a_region_of_interest_with_a_row_pitch(pad, monkeypatch):
    """Rows `stride` bytes apart (the bytes between them poisoned), through the C ABI, with the per-level launches: every padded level
    and the results equal the oracle's on the contiguous copy."""
    from orb_slam2_e_amd._lib import check
    monkeypatch.setenv("ORBX_PYR_CHAIN_MAX_BATCH", "0")
    h, w = HEIGHT, 258
    img = _frames(1, h, w, 5)[0]
    (okps, odesc, olevels), = _reference([img], FOUR)
    stride = w + pad
    buf = np.full((h - 1) * stride + w, 0xA5, np.uint8)
    for y in range(h):
        buf[y * stride: y * stride + w] = img[y]
    ex = ORBextractor(*FOUR)
    ex._reserve(w, h, 1)
    kps = np.zeros(ex.capacity, KP_DTYPE); desc = np.zeros((ex.capacity, 32), np.uint8); n = C.c_int(0)
    check(ex._L.orbx_extract(ex._h, buf.ctypes.data_as(C.c_void_p), w, h, stride, kps.ctypes.data_as(C.c_void_p),
                             desc.ctypes.data_as(C.c_void_p), ex.capacity, C.byref(n)))
    for l in range(4):
        assert np.array_equal(ex.pyramid_level(0, l, padded=True), olevels[l]), l
    _same_keypoints(kps[:n.value], okps)
    assert np.array_equal(desc[:n.value], odesc)
