"""Small hand-built images for the extractor chain (k_pyr*, k_blur, k_fast_cells, k_octree, k_describe): content at the extremes
that seeded rectangles, discs and noise never reach.  Every scene has a name, a purpose and its extractor parameters; it is built
from a seed or by construction, and never modified afterwards (the arrays are read-only).  tests/test_cpu_extract_reference.py
asserts on the numpy restatement that each scene reaches what it is for; tests/test_gpu_extract_content.py runs them on the device.

Sizes: 200 x 260 (rows x columns) with 4 levels at scale 1.2; one 88 x 87 single-cell image and one 120 x 150 noise
image with one level; one 207 x 255."""
import collections
import functools

import numpy as np

Scene = collections.namedtuple("Scene", "name purpose image params info")

H, W = 200, 260
PARAMS = (300, 1.2, 4, 20, 7)
LATTICE_PARAMS = (186, 1.2, 4, 20, 7)             # level-0 quota 60 against several hundred equal candidates
BLOCK = 40                                        # marks stand at the centres of 40-px blocks: further apart than a 31-px patch
EDGE_CONTRASTS = (6, 7, 8, 19, 20, 21, 22)        # either side of minThFAST = 7 (|c| - 1 >= 7) and iniThFAST = 20 (|c| - 1 >= 20)
GROUNDS = (100, 0, 3, 252, 255)
NOISE_HALF_SEED = 12                              # found by trying seeds 1, 2, ...: about one image in ten has such a keypoint


def _ro(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


def binary_blocks(h=H, w=W, seed=1, n=260):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    for _ in range(n):
        sw, sh = (int(v) for v in rng.integers(1, 41, 2))
        x, y = int(rng.integers(-sw // 2, w - sw // 2)), int(rng.integers(-sh // 2, h - sh // 2))
        img[max(y, 0):max(y + sh, 0), max(x, 0):max(x + sw, 0)] = 255 * int(rng.integers(0, 2))
    return img


def stripes(h=H, w=W):
    img = np.zeros((h, w), np.uint8)
    img[:h // 2, 1::2] = 255                       # 1-px columns in the top half
    img[h // 2 + 1::2, :] = 255                    # 1-px rows in the bottom half
    return img


def checker(h=H, w=W, side=8):
    yy, xx = np.mgrid[0:h, 0:w]
    return (255 * (((yy // side) + (xx // side)) & 1)).astype(np.uint8)


def lattice(h=H, w=W, ground=100, value=160, pitch=7, x0=0, y0=0):
    img = np.full((h, w), ground, np.uint8)
    img[y0::pitch, x0::pitch] = value
    return img


def _centre(bx, by, x0=0, y0=0):
    return x0 + bx * BLOCK + BLOCK // 2, y0 + by * BLOCK + BLOCK // 2


def threshold_edges(ground, h=H, w=W):
    """Single pixels of contrast c, one per 40-px block, and 3 x 3 dots.  Every block row of a 200-row image lies in a FAST cell
    row of its own (34-px cells from 16: the centres 20, 60, 100, 140, 180 fall in cell rows 0 .. 4), so the weak contrasts
    (|c| <= 20: block rows 0 - 2) share no cell with a strong one and their cells fall back to minThFAST; the strong ones
    (|c| >= 21) stand in block rows 3 and 4.  Returns the image and the marks: (x, y, c, kind)."""
    signs = [s for s in (1, -1) if 0 <= ground + s * 22 <= 255]
    img = np.full((h, w), ground, np.int16)
    weak = [(s * c, "pixel") for c in EDGE_CONTRASTS if c <= 20 for s in signs] + [(s * 20, "dot") for s in signs] + \
           [(s * 8, "dot") for s in signs]
    strong = [(s * c, "pixel") for c in EDGE_CONTRASTS if c > 20 for s in signs] + [(s * 22, "dot") for s in signs] + \
             [(s * 90, "dot") for s in signs]
    per_row = w // BLOCK
    assert len(weak) <= 3 * per_row and len(strong) <= 2 * per_row
    marks = []
    for k, (c, kind) in enumerate(weak):
        marks.append(_centre(k % per_row, k // per_row) + (c, kind))
    for k, (c, kind) in enumerate(strong):
        marks.append(_centre(k % per_row, 3 + k // per_row) + (c, kind))
    for x, y, c, kind in marks:
        r = 1 if kind == "dot" else 0
        img[y - r:y + r + 1, x - r:x + r + 1] = ground + c
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8), marks


# a mark: ((dx, dy, value above the ground), ...) round its keypoint at (0, 0); the end pixel is brighter than the body, so strict
# non-maximum suppression keeps it (the body's corner pixels have equal scores and remove each other)
def _arm(dx, dy, n=9, body=60):
    return [(k * dx, k * dy, body) for k in range(1, n)]


MARKS = collections.OrderedDict([
    ("pixel", []),                                                  # m10 == m01 == 0
    ("line +x", _arm(1, 0)), ("line +y", _arm(0, 1)), ("line -x", _arm(-1, 0)), ("line -y", _arm(0, -1)),
    ("corner +x+y", _arm(1, 0) + _arm(0, 1)), ("corner -x+y", _arm(-1, 0) + _arm(0, 1)),
    ("corner -x-y", _arm(-1, 0) + _arm(0, -1)), ("corner +x-y", _arm(1, 0) + _arm(0, -1)),
])
MARK_ANGLES = {"line +x": 0.0, "line +y": 90.0, "line -x": 180.0, "line -y": 270.0}


def draw_mark(img, x, y, kind, ground, end=100):
    for dx, dy, v in MARKS[kind]:
        img[y + dy, x + dx] = ground + v
    img[y, x] = ground + end


def symmetric_marks(h=H, w=W, ground=100):
    """Marks that are symmetric about an axis or a diagonal through their keypoint, on a flat ground: moments with m01 == 0,
    m10 == 0, |m10| == |m01| and both 0.  Returns the image and (x, y, kind) per mark."""
    img = np.full((h, w), ground, np.uint8)
    kinds = list(MARKS) + ["pixel", "pixel", "pixel", "line +x", "line +y", "line -x", "line -y", "corner +x+y", "corner -x-y"]
    per_row = w // BLOCK
    marks = []
    for k, kind in enumerate(kinds):
        x, y = _centre(k % per_row, k // per_row)
        draw_mark(img, x, y, kind, ground)
        marks.append((x, y, kind))
    return img, marks


def mixed(h, w, seed):
    """The same content kinds in one image of any size: binary blocks on the left, a lattice patch, marks and weak pixels."""
    img = np.full((h, w), 100, np.uint8)
    img[:, :w // 3] = binary_blocks(h, w // 3, seed, n=40)
    img[h // 2:, w // 3:] = lattice(h - h // 2, w - w // 3)
    img[h // 2 - 4:h // 2, w // 3:] = 100
    marks = []
    x0, y0 = w // 3 + 20, 22
    for k, kind in enumerate(("corner +x+y", "line -x", "pixel", "corner -x-y", "line +y")):
        x = x0 + k * 36
        if x + 12 < w:
            draw_mark(img, x, y0, kind, 100)
            marks.append((x, y0, kind))
    return img, marks


@functools.lru_cache(maxsize=None)
def scenes():
    out = [
        Scene("binary_blocks", "blurred pixels of exactly 0 and 255, row sums at both ends of 16 bits, the 257-tap clamp; 0 and 255 "
              "in every pyramid level", _ro(binary_blocks()), PARAMS, None),
        Scene("stripes", "1-px 0 / 255 columns (top) and rows (bottom): the largest differences between neighbours in the resize "
              "and in the blur's two directions", _ro(stripes()), PARAMS, None),
        Scene("checker8", "an 8-px 0 / 255 checkerboard: many candidates of equal response above level 0", _ro(checker()), PARAMS,
              None),
        Scene("lattice", "equal single pixels every 7 px: hundreds of candidates with ONE response against a quota of 60 -- first "
              "candidate wins every leaf, later-created node first among equals", _ro(lattice()), LATTICE_PARAMS, None),
        Scene("lattice3", "the lattice with 3 levels (other quotas, another split order)", _ro(lattice()), (186, 1.2, 3, 20, 7), None),
    ]
    for g in GROUNDS:
        img, marks = threshold_edges(g)
        out.append(Scene("threshold_edges_%d" % g, "single pixels of contrast 6 .. 22 and 3 x 3 dots on ground %d: > against >= at "
                         "iniThFAST / minThFAST, the fallback, the NMS tie, v +- t outside the byte range" % g, _ro(img), PARAMS,
                         tuple(marks)))
    img, marks = symmetric_marks()
    out.append(Scene("symmetric_marks", "line ends, diagonal corners and single pixels: angles of exactly 0 / 90 / 180 / 270, "
                     "|m10| == |m01|, m10 == m01 == 0", _ro(img), PARAMS, tuple(marks)))
    img, marks = mixed(88, 87, 5)
    out.append(Scene("single_cell", "88 x 87, one level: a single FAST cell with the same content kinds", _ro(img), (200, 1.2, 1, 12, 5),
                     tuple(marks)))
    out.append(Scene("noise_half", "120 x 150 uniform noise, one level, seed %d: among its ~950 keypoints one samples the blurred image at "
                     "a coordinate of exactly k + 1/2 with k even, and the pixel one further differs -- computeOrbDescriptor's cvRound "
                     "has to round half to even (no resize here: nothing else rounds)" % NOISE_HALF_SEED,
                     _ro(np.random.default_rng(NOISE_HALF_SEED).integers(0, 256, (120, 150), dtype=np.uint8)), (1000, 1.2, 1, 20, 7), None))
    img, marks = mixed(207, 255, 6)
    out.append(Scene("odd_sizes", "207 x 255: odd sizes at every level with the same content kinds; 255 / 1.2 = 212.5 and 207 / 1.2 = 172.5 exactly in "
                     "float32, so cvRound's half-to-even rule decides the size of level 1 (212 x 172)", _ro(img), PARAMS, tuple(marks)))
    return tuple(out)


def by_name(name):
    return {s.name: s for s in scenes()}[name]


@functools.lru_cache(maxsize=None)
def restated(name):
    """The numpy restatement's result for a scene (extract_reference.run): computed once, shared, never modified."""
    import extract_reference
    s = by_name(name)
    return extract_reference.run(s.image, s.params)


class OracleResult:
    pass


def oracle_run(image, params):
    """The C oracle's stages in the shape of extract_reference.Result: .padded[l], .blurred[blur_variant][l], .cands[l], .kps[l],
    .out[(blur_variant, trig_variant)]."""
    import oracle
    import extract_reference
    res = OracleResult()
    res.out, res.blurred = {}, {}
    for bv in (0, 1):
        for tv in (0, 1):
            o = oracle.OrbOracle(*params)
            o.set_blur_taps(extract_reference.TAPS[bv])
            o.set_trig_variant(tv)
            res.out[(bv, tv)] = o.extract(image)
            if tv == 0:
                res.blurred[bv] = [o.level_blurred(l) for l in range(params[2])]
            if (bv, tv) == (0, 0):
                res.padded = [o.level_padded(l)[:, :o.level_dims(l)[0] + 38] for l in range(params[2])]
                res.cands = [o.level_cands(l) for l in range(params[2])]
                res.kps = [o.level_kps(l) for l in range(params[2])]
    return res


@functools.lru_cache(maxsize=None)
def oracled(name):
    s = by_name(name)
    return oracle_run(s.image, s.params)
