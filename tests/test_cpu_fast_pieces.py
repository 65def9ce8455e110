"""k_fast_cells loads a cell's tile as 16-byte pieces, and the last piece of a row reads up to 12 bytes past the dwords the tile needs.
Host plan only (orbx_debug_fast_pieces, no GPU): over a sweep of frame sizes and scales every piece of every cell lies inside its
level's padded row, inside the level's rows and inside the frame's pyramid block -- the geometry restated here from the level sizes
alone (stride = 32 + w + 19 rounded up to 64, 19 border rows, levels 256-byte aligned), not taken from the planner."""
import numpy as np
import pytest

from orb_slam2_e_amd.extractor import FAST_PIECE_FIELDS, fast_pieces, plan

PADX, EDGE = 32, 19
WIDTHS = list(range(62, 701, 7))            # 7 is odd: every residue mod 64 of a row's first pixel comes up
HEIGHTS = (62, 77, 131, 480, 700)           # those up to the width, the square and a frame slightly taller than wide (the planner refuses aspect ratios below 0.5)
SCALES = (1.1, 1.2, 1.5, 2.0)
COL = {n: i for i, n in enumerate(FAST_PIECE_FIELDS)}


def _levels(scale, w, h):
    """as many levels (at most 8) as stay at or above 62 px, the smallest the planner takes"""
    n, s = 1, np.float32(1.0)
    while n < 8:
        s = np.float32(s * np.float32(scale))
        if min(w, h) / float(s) < 63:
            break
        n += 1
    return n


def _check(w, h, scale):
    nl = _levels(scale, w, h)
    params = (500, scale, nl, 20, 7)
    info = plan(*params, w, h)
    cells = fast_pieces(*params, w, h)
    assert len(cells) == sum(info["level_cells"]) == info["cells_per_frame"]
    # the frame's block, from the level sizes alone
    strides, offs, off = [], [], 0
    for lw, lh in zip(info["level_w"], info["level_h"]):
        strides.append((PADX + lw + EDGE + 63) & ~63)
        offs.append(off)
        off = (off + strides[-1] * (lh + 2 * EDGE) + 255) & ~255
    assert off == info["frame_bytes"]
    lv = cells[:, COL["level"]]
    stride, loff = np.asarray(strides)[lv], np.asarray(offs)[lv]
    lw, lh = np.asarray(info["level_w"])[lv], np.asarray(info["level_h"])[lv]
    assert np.array_equal(cells[:, COL["stride"]], stride)
    rel = cells[:, COL["img_off"]] - loff
    row0, col0 = rel // stride, rel % stride
    rows, pieces, cw = cells[:, COL["rows"]], cells[:, COL["pieces"]], cells[:, COL["cw"]]
    live = rows > 0
    assert live.any() and np.array_equal(live, pieces > 0)
    # the tile's first byte is level pixel (x0 - 5, y0), and the pieces cover the dwords the tile takes
    assert np.array_equal(col0, PADX + cells[:, COL["x0"]] - 5) and np.array_equal(row0, cells[:, COL["y0"]] + EDGE)
    assert (16 * pieces[live] >= 4 * ((cw[live] + 8) >> 2)).all() and (16 * (pieces[live] - 1) < 4 * ((cw[live] + 8) >> 2)).all()
    col1, row1 = col0 + 16 * pieces, row0 + rows
    assert (col0[live] >= 0).all() and (col1[live] <= stride[live]).all(), "a piece leaves the padded row"
    assert (col1[live] <= PADX + lw[live] + EDGE).all(), "a piece reads the row's unwritten padding"
    assert (row0[live] >= 0).all() and (row1[live] <= lh[live] + 2 * EDGE).all(), "a row outside the level"
    last = cells[:, COL["img_off"]].astype(np.int64) + (rows - 1).astype(np.int64) * stride + 16 * pieces
    assert (last[live] <= info["frame_bytes"]).all(), "a piece behind the frame's block"
    return int((PADX + lw[live] + EDGE - col1[live]).min())


@pytest.mark.parametrize("scale", SCALES)
def test_every_piece_lies_in_its_padded_row_and_in_the_frame(scale):
    slack = min(_check(w, h, scale) for w in WIDTHS for h in sorted({x for x in HEIGHTS if x <= w} | {w, w + 9}))
    # (the grid keeps every cell 16 px inside the level: a piece ends at least 20 bytes before the end of the border)
    assert slack >= EDGE + 1


def test_the_three_tile_variants_and_their_widest_cells():
    """one level, one cell column: cell widths 44 / 45 / 52 / 53 / 59 at the edges of the 52-, 64- and 80-byte tile rows"""
    for w, cw, ts in ((62, 30, 52), (76, 44, 52), (77, 45, 64), (84, 52, 64), (85, 53, 80), (91, 59, 80)):
        params = (200, 1.2, 1, 20, 7)
        cells = fast_pieces(*params, w, 75)
        assert cells[:, COL["cw"]].max() == cw and plan(*params, w, 75)["fast_tile_stride"] == ts, (w, cw, ts)
        _check(w, 75, 1.2)
