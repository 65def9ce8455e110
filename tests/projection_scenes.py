"""Scenes for the projection prefix of the SearchByProjection family at its boundaries (tests/projection_reference.py), shared
by the CPU and the GPU tests.  Numpy only, seeded: identical wherever they are generated.

Geometry: the camera looks down +z with Rcw = I; map points are placed at Ow + PO with small dyadic PO, so Rcw * P + tcw, P - Ow
and the norms are exact and the free input of each boundary (mind, maxd, the normal, a bound, th) can be set to the float that
sits on it.  A boundary pair is two entries that differ in one input by one float ulp and, by the restatement, in their outcome;
_edge finds that pair by bisection over the ordered floats.  Degenerate entries: PcZ = +0 and -0 (u infinite or NaN), a point at
the camera centre with mind 0 (dist 0: the ratio of PredictScale is +inf), mind / maxd 0, maxd = +inf, NaN positions and bounds.
"""
import numpy as np

import projection_reference as R

f32 = np.float32
PYRAMIDS = {"ref": (1.2, 8), "fork": (1.1, 6)}   # the reference's (ORBextractor.scaleFactor / nLevels) and the fork's launch files
CAM = (500.0, 500.0, 320.0, 240.0)
BOUNDS = (0.0, 0.0, 640.0, 480.0)
OW = np.array([0.5, -0.25, 1.0], f32)
DZ = f32(2.0)           # project_points: tcw = -Ow + (0, 0, DZ), so that a point at Ow projects to the image centre


def pyramid(name):
    s, n = PYRAMIDS[name]
    sf = np.array([1.0], f32)
    for _ in range(1, n):
        sf = np.append(sf, f32(sf[-1] * f32(s)))
    return sf, f32(np.log(f32(s)))


def _ord(x):
    i = int(np.array(x, f32).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _unord(k):
    return np.array(k if k >= 0 else (-k) | -0x80000000, np.int32).view(f32)[()]


def _edge(fn, lo, hi):
    """Adjacent floats a < b between lo and hi with fn(a) == fn(lo) != fn(b)."""
    a, b = _ord(f32(lo)), _ord(f32(hi))
    fa = fn(_unord(a))
    assert fn(_unord(b)) != fa, "no boundary between the two ends"
    while b - a > 1:
        m = (a + b) // 2
        if fn(_unord(m)) == fa:
            a = m
        else:
            b = m
    return _unord(a), _unord(b)


class Entries:
    """Parallel lists of map-point entries; pairs = (i, j, boundary name) of boundary pairs."""

    def __init__(self):
        self.pos, self.nrm, self.mind, self.maxd, self.octave, self.valid, self.tag = [], [], [], [], [], [], []
        self.pairs = []

    def add(self, po, nrm=(0.0, 0.0, 1.0), mind=0.5, maxd=40.0, octave=0, valid=1, tag="", origin=OW):
        self.pos.append(np.array(origin, f32) + np.array(po, f32)); self.nrm.append(np.array(nrm, f32))
        self.mind.append(f32(mind)); self.maxd.append(f32(maxd)); self.octave.append(int(octave)); self.valid.append(int(valid))
        self.tag.append(tag)
        return len(self.pos) - 1

    def pair(self, name, a, b, **kw):
        i = self.add(tag=name, **{**kw, **a}); j = self.add(tag=name, **{**kw, **b})
        self.pairs.append((i, j, name))

    def arrays(self):
        return dict(pos=np.array(self.pos, f32).reshape(-1, 3), nrm=np.array(self.nrm, f32).reshape(-1, 3),
                    mind=np.array(self.mind, f32), maxd=np.array(self.maxd, f32), octave=np.array(self.octave, np.int32),
                    valid=np.array(self.valid, np.uint8), tag=list(self.tag), pairs=list(self.pairs))


def _pp(mode, sf, ls, th, po, nrm, mind, maxd, t=None):
    """The restated outcome of one project_points entry: (code, level, r bits)."""
    tcw = -OW + np.array([0, 0, DZ], f32) if t is None else t
    out, q, code, _ = R.project_points(mode, [OW + np.array(po, f32)], [nrm], [mind], [maxd], np.eye(3, dtype=f32), tcw, OW, CAM,
                                       BOUNDS, 40.0, 0.5, ls, sf, th)
    return int(code[0]), int(out["level"][0]), int(q["r"].view(np.uint32)[0])


def _common_degenerate(E, extra_nan=True):
    inf = np.inf
    E.add((0.0, 0.0, 1.5), mind=0.0, maxd=inf, tag="maxd_inf")                  # ratio +inf: level 0 on x86-64
    E.add((0.125, -0.25, 3.0), mind=0.5, maxd=inf, tag="maxd_inf")
    E.add((0.0, 0.0, 1.5), mind=0.0, maxd=3.0e38, tag="maxd_huge")              # 1.2f * maxd overflows to +inf
    E.add((0.0, 0.0, 2.0), mind=0.0, maxd=0.0, tag="maxd_0")                    # ratio 0: logf -inf
    E.add((0.25, 0.0, 2.0), mind=0.0, maxd=np.nan, tag="maxd_nan")
    E.add((0.25, 0.0, 2.0), mind=np.nan, maxd=20.0, tag="mind_nan")
    if extra_nan:
        E.add((np.nan, 0.0, 2.0), tag="pos_nan")
        E.add((0.0, 0.0, np.nan), tag="pos_nan")


def frustum_scene(mode, pyr="ref", th=1.0):
    """Entries for orbm_project_points (mode 0 isInFrustum, 1 / 2 the Fuse forms), the call's tcw = -Ow + (0, 0, DZ)."""
    sf, ls = pyramid(pyr)
    nl = len(sf)
    E = Entries()
    ax = (0.0, 0.0, 3.0)
    fn = lambda k: (lambda x: _pp(mode, sf, ls, th, **{**dict(po=ax, nrm=(0, 0, 1), mind=0.5, maxd=40.0), k: x})[0])
    # dist around the scale-invariance range: mind and maxd one ulp either side (dist = 3 exactly)
    a, b = _edge(fn("mind"), 0.5, 10.0); E.pair("near", dict(po=ax, mind=a), dict(po=ax, mind=b))
    a, b = _edge(fn("maxd"), 0.5, 40.0); E.pair("far", dict(po=ax, maxd=a), dict(po=ax, maxd=b))
    # the same at distances that are not powers of two times small integers (the 0.9 / 0.8 products then round)
    for z in (1.7, 2.3, 2.9, 3.1, 3.7, 4.3, 5.1, 6.7):
        pz = (0.0, 0.0, float(f32(z)))
        g = lambda k: (lambda x: _pp(mode, sf, ls, th, **{**dict(po=pz, nrm=(0, 0, 1), mind=0.5, maxd=40.0), k: x})[0])
        a, b = _edge(g("mind"), 0.3, 20.0); E.pair("near", dict(po=pz, mind=a), dict(po=pz, mind=b))
        a, b = _edge(g("maxd"), 0.3, 40.0); E.pair("far", dict(po=pz, maxd=a), dict(po=pz, maxd=b))
    # PredictScale's steps: maxd around dist * scale^k, k = 1 .. nl - 1 and the clamp to nl - 1
    lvl = lambda x: _pp(mode, sf, ls, th, ax, (0, 0, 1), 0.01, x)[1]
    for k in range(1, nl):
        lo, hi = f32(3.0 * float(sf[k - 1]) * 0.9999), f32(3.0 * float(sf[k - 1]) * 1.0001)
        a, b = _edge(lvl, lo, hi); E.pair(f"level{k}", dict(po=ax, mind=0.01, maxd=a), dict(po=ax, mind=0.01, maxd=b))
    E.add(ax, mind=0.01, maxd=3.0 * float(sf[-1]) * 4, tag="level_high")
    # the viewing angle: a point off the axis with a small z component in PO, its normal's z swept
    po = (1.5, 0.0, 0.375)
    cos_code = lambda x: _pp(mode, sf, ls, th, po, (0.6, 0.0, x), 0.5, 40.0)[0]
    if mode == 0:
        a, b = _edge(cos_code, -0.9, 0.99); E.pair("cos_limit", dict(po=po, nrm=(0.6, 0, a)), dict(po=po, nrm=(0.6, 0, b)))
        # RadiusByViewingCos: viewCos = nz exactly on the axis; 0.998 in double lies between two floats
        lo = np.nextafter(f32(0.998), f32(0)) if float(f32(0.998)) > 0.998 else f32(0.998)
        E.pair("radius", dict(po=ax, nrm=(0, 0, lo)), dict(po=ax, nrm=(0, 0, np.nextafter(lo, f32(1)))))
        po2 = (0.5, 0.0, 0.03125)
        rad = lambda x: _pp(mode, sf, ls, th, po2, (0.998, 0.0, x), 0.5, 40.0)[0]
        a, b = _edge(rad, 0.0, 0.2); E.pair("radius_offaxis", dict(po=po2, nrm=(0.998, 0, a)), dict(po=po2, nrm=(0.998, 0, b)))
    else:
        a, b = _edge(cos_code, -0.9, 0.99); E.pair("dot_half", dict(po=po, nrm=(0.6, 0, a)), dict(po=po, nrm=(0.6, 0, b)))
        # the clamp to level 0: dist just inside 1.2f * maxd (ratio ~ 1 / 1.2: ceil(-1.91) = -1 on the fork's pyramid)
        a, b = _edge(fn("maxd"), 2.0, 3.0)
        E.add(ax, maxd=b, tag="level_low")
    # degenerate points
    E.add((0.0, 0.0, 0.0), mind=0.0, maxd=20.0, tag="centre")                   # P = Ow: dist 0, ratio +inf
    E.add((0.0, 0.0, -2.0), nrm=(0.0, 0.0, -1.0), tag="z_pos0")                 # PcZ = +0, u NaN (0 * inf)
    E.add((0.25, 0.0, -2.0), tag="z_pos0_inf")                                  # PcZ = +0, u +inf
    E.add((0.0, 0.0, -2.5), tag="behind")
    E.add((0.0, 2.0, 1.0), tag="out_v")
    _common_degenerate(E)
    for k in range(4):                                                          # a few ordinary points
        E.add((0.3 * k - 0.5, 0.2 * k - 0.3, 2.0 + k), nrm=(0.1, 0.0, 0.99), mind=0.5, maxd=40.0, tag="plain")
    d = E.arrays()
    d.update(mode=mode, pyr=pyr, sf=sf, ls=ls, th=f32(th), cam=CAM, bounds=BOUNDS, Rcw=np.eye(3, dtype=f32),
             tcw=(-OW + np.array([0, 0, DZ], f32)).astype(f32), Ow=OW.copy(), mbf=f32(40.0), cos_limit=f32(0.5))
    return d


def minus_zero_scene(mode):
    """PcZ = -0: a point whose row sums are all -0 (x, y < 0 in front of -0 weights) and tcw[2] = -0."""
    sf, ls = pyramid("ref")
    pos = np.array([[-0.0, -0.0, -0.0], [-1.0, -1.0, -0.0], [0.5, -0.5, -0.0]], f32)
    tcw = np.array([0.0, 0.0, -0.0], f32)
    return dict(mode=mode, pos=pos, nrm=np.tile(np.array([0, 0, 1], f32), (3, 1)), mind=np.zeros(3, f32),
                maxd=np.full(3, 10.0, f32), Rcw=np.eye(3, dtype=f32), tcw=tcw, Ow=np.zeros(3, f32), cam=CAM, bounds=BOUNDS,
                mbf=f32(40.0), cos_limit=f32(0.5), ls=ls, sf=sf, th=f32(1.0))


def project_bounds_variants(sc):
    """Bounds that sit on the computed u / v of the first plain entry, and one ulp inside: (name, bounds4, entry)."""
    i = sc["tag"].index("plain")
    out, q, code, _ = R.project_points(sc["mode"], sc["pos"][i:i + 1], sc["nrm"][i:i + 1], sc["mind"][i:i + 1], sc["maxd"][i:i + 1],
                                       sc["Rcw"], sc["tcw"], sc["Ow"], sc["cam"], sc["bounds"], sc["mbf"], sc["cos_limit"], sc["ls"],
                                       sc["sf"], sc["th"])
    u, v = f32(out["u"][0]), f32(out["v"][0])
    up, dn = lambda x: np.nextafter(x, f32(np.inf)), lambda x: np.nextafter(x, f32(-np.inf))
    b = [f32(x) for x in sc["bounds"]]
    return [("max_x=u", (b[0], b[1], u, b[3])), ("max_x=u-", (b[0], b[1], dn(u), b[3])), ("max_x=u+", (b[0], b[1], up(u), b[3])),
            ("min_x=u", (u, b[1], b[2], b[3])), ("min_x=u+", (up(u), b[1], b[2], b[3])),
            ("max_y=v", (b[0], b[1], b[2], v)), ("max_y=v-", (b[0], b[1], b[2], dn(v))), ("max_y=v+", (b[0], b[1], b[2], up(v))),
            ("min_y=v", (b[0], v, b[2], b[3])), ("min_y=v+", (b[0], up(v), b[2], b[3])), ("nan", (b[0], b[1], f32(np.nan), b[3]))], i


# ------------------------------------------------------------------------------------------------ the whole-search forms
def _frame(rng, n, sf, stereo):
    kps = np.zeros(n, R_KP)
    kps["x"] = rng.uniform(2, 638, n); kps["y"] = rng.uniform(2, 478, n)
    kps["octave"] = rng.integers(0, len(sf), n); kps["angle"] = rng.uniform(0, 360, n).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur = np.where(rng.random(n) < 0.7, kps["x"] - rng.uniform(1, 30, n), -1.0).astype(f32) if stereo else None
    return kps, desc, ur


R_KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                 ("class_id", "<i4")])


def form_scene(seed, pyr="ref", stereo=False, motion="none", th=7.0):
    """A key frame / current frame at pose Tcw = [I | -Ow] and map points for LAST, KF, SIM3 and PAIR: boundary pairs of the
    distance range and of PredictScale's steps (dist = 3 on the optical axis), points aimed at keypoints (so the searches match),
    the degenerate points, a point at the camera centre.  Tlw moves the last frame along z by motion * 3 mb."""
    rng = np.random.default_rng(seed)
    sf, ls = pyramid(pyr)
    nl = len(sf)
    mb, mbf = f32(0.08), f32(40.0)
    Tcw = np.eye(4, dtype=f32); Tcw[:3, 3] = -OW
    Tlw = Tcw.copy(); Tlw[2, 3] = f32(Tlw[2, 3] - f32({"forward": 3.0, "backward": -3.0, "none": 0.25}[motion] * mb))
    n = 600
    kps, desc, ur = _frame(rng, n, sf, stereo)
    E = Entries()
    ax = (0.0, 0.0, 3.0)

    def kf(key):
        def f(x):
            kw = {**dict(mind=0.5, maxd=40.0), key: x}
            return int(R.form_kf(Tcw, [1], [OW + np.array(ax, f32)], [kw["mind"]], [kw["maxd"]], CAM, BOUNDS, sf, ls, th)[1][0])
        return f
    a, b = _edge(kf("mind"), 0.5, 10.0); E.pair("near", dict(po=ax, mind=a), dict(po=ax, mind=b))
    a, b = _edge(kf("maxd"), 0.5, 40.0); E.pair("far", dict(po=ax, maxd=a), dict(po=ax, maxd=b))
    E.add(ax, maxd=b, tag="level_low")
    lvl = lambda x: int(R.form_kf(Tcw, [1], [OW + np.array(ax, f32)], [0.01], [x], CAM, BOUNDS, sf, ls, th)[0]["min_level"][0])
    for k in range(1, nl):
        lo, hi = f32(3.0 * float(sf[k - 1]) * 0.9999), f32(3.0 * float(sf[k - 1]) * 1.0001)
        a, b = _edge(lvl, lo, hi); E.pair(f"level{k}", dict(po=ax, mind=0.01, maxd=a), dict(po=ax, mind=0.01, maxd=b))
    E.add(ax, mind=0.01, maxd=3.0 * float(sf[-1]) * 4, tag="level_high")
    # the Sim3 form's dot < 0.5 dist: the normal's z swept on an off-axis point
    po = (1.5, 0.0, 3.0)
    sim3 = lambda x: int(R.form_sim3(Tcw, [1], [OW + np.array(po, f32)], [(0.2, 0.0, x)], [0.5], [40.0], CAM, BOUNDS, sf, ls, th)[1][0])
    a, b = _edge(sim3, -0.9, 0.99); E.pair("dot_half", dict(po=po, nrm=(0.2, 0, a)), dict(po=po, nrm=(0.2, 0, b)))
    # points aimed at keypoints (the searches then match), some at a camera-centre distance of exactly mind * 0.8
    aim = rng.choice(n, 160, replace=False)
    fx, fy, cx, cy = CAM
    for j in aim:
        z = f32(rng.uniform(1.0, 6.0))
        x = f32((kps["x"][j] + rng.normal(0, 1.0) - cx) / fx * z); y = f32((kps["y"][j] + rng.normal(0, 1.0) - cy) / fy * z)
        E.add((x, y, z), nrm=(0.0, 0.0, 1.0), mind=0.3, maxd=f32(z * rng.uniform(1.0, 9.0)), octave=int(kps["octave"][j]),
              valid=int(rng.random() < 0.9), tag="aimed")
    E.add((0.0, 0.0, 0.0), mind=0.0, maxd=20.0, tag="centre")                   # P = Ow: PcZ = +0 (u NaN), dist 0, ratio +inf
    E.add((0.25, 0.0, 0.0), mind=0.0, maxd=20.0, tag="z_pos0_inf")
    E.add((0.0, 0.0, -2.5), tag="behind")
    E.add((0.0, 2.0, 1.0), tag="out_v")
    E.add((0.125, 0.0, 3.0), mind=10.0, tag="near_pair")                        # too near in key frame 2 as well
    E.add((0.5, 0.0, 1.0), tag="invalid", valid=0)
    _common_degenerate(E)
    d = E.arrays()
    d["octave"] = np.minimum(d["octave"], nl - 1).astype(np.int32)
    d["angle"] = rng.uniform(0, 360, len(d["pos"])).astype(f32)
    d["mp_desc"] = rng.integers(0, 256, (len(d["pos"]), 32), dtype=np.uint8)
    j_of = {}                                                                   # aimed points: the keypoint's descriptor, a few bits off
    k = 0
    for i, t in enumerate(d["tag"]):
        if t == "aimed":
            j = aim[k]; k += 1
            d["mp_desc"][i] = desc[j] ^ np.packbits(rng.random(256) < 0.05, bitorder="little")
            d["angle"][i] = f32((kps["angle"][j] + (12.0 if k % 3 else 95.0)) % 360)
            j_of[i] = j
    occ = (rng.random(n) < 0.1).astype(np.uint8)
    # SearchBySim3: key frame 2 at pose T2w (shifted along x), the transform between them exact
    T2w = Tcw.copy(); T2w[0, 3] = f32(T2w[0, 3] - f32(0.125))
    s12 = f32(1.0); R12 = np.eye(3, dtype=f32); t12 = np.array([0.125, 0.0, 0.0], f32)
    kps2, desc2, _ = _frame(rng, n, sf, False)
    d.update(pyr=pyr, sf=sf, ls=ls, nl=nl, th=f32(th), cam=CAM, bounds=BOUNDS, mb=mb, mbf=mbf, Tcw=Tcw, Tlw=Tlw, Scw=Tcw.copy(),
             T2w=T2w, s12=s12, R12=R12, t12=t12, kps=kps, desc=desc, uright=ur, occupied=occ, kps2=kps2, desc2=desc2,
             stereo=stereo, motion=motion)
    return d


# --------------------------------------------------------------------------------------------------------------- windows
def window_scene(seed=0):
    """Keypoints on a lattice 40 px apart (one per window at most), each probed by queries whose centre puts it exactly at
    |dx| = r, one ulp inside and outside, likewise |dy|, the level range's ends and the stereo test's |xr - uright| = r.
    Query i's descriptor equals its target keypoint's, every other descriptor is far: a search's best is the target or none."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(30.0, 620.0, 40.0), np.arange(30.0, 460.0, 40.0))
    n = xs.size
    kps = np.zeros(n, R_KP)
    kps["x"] = (xs.ravel() + rng.uniform(-3, 3, n)).astype(f32); kps["y"] = (ys.ravel() + rng.uniform(-3, 3, n)).astype(f32)
    kps["octave"] = rng.integers(0, 8, n); kps["angle"] = rng.uniform(0, 360, n).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur = np.where(rng.random(n) < 0.8, kps["x"] - f32(12.5), -1.0).astype(f32)
    qs, target, tags = [], [], []
    up, dn = lambda x: np.nextafter(f32(x), f32(np.inf)), lambda x: np.nextafter(f32(x), f32(-np.inf))
    for j in range(n):
        x, y, o = f32(kps["x"][j]), f32(kps["y"][j]), int(kps["octave"][j])
        r = f32(rng.choice([3.0, 4.5 * 1.2, 7.0 * 1.44, 15.0]))
        xr = f32(ur[j]) if ur[j] > 0 else f32(0)
        kind = j % 6
        if kind == 0:      # u = x - r (dx = r: out), and one ulp either side of the centre that makes dx = r
            for u in (f32(x - r), up(f32(x - r)), dn(f32(x - r)), f32(x + r), dn(f32(x + r))):
                qs.append((u, y, r, xr, o - 1, o)); target.append(j); tags.append("dx")
        elif kind == 1:
            for v in (f32(y - r), up(f32(y - r)), f32(y + r), dn(f32(y + r)), up(f32(y + r))):
                qs.append((x, v, r, xr, o - 1, o)); target.append(j); tags.append("dy")
        elif kind == 2:    # the level range: min_level = octave + 1 / octave, max_level = octave - 1 / octave; -1 / -1 off
            for lo, hi in ((o + 1, o + 1), (o, o), (o - 1, o - 1), (-1, -1), (0, -1), (1, -1), (o, -1), (o + 1, -1)):
                qs.append((x, y, r, xr, lo, hi)); target.append(j); tags.append("level")
        elif kind == 3:    # the stereo test: xr = uright +- r, one ulp outside
            if ur[j] > 0:
                for q in (f32(ur[j] + r), up(f32(ur[j] + r)), f32(ur[j] - r), dn(f32(ur[j] - r))):
                    qs.append((x, y, r, q, -1, -1)); target.append(j); tags.append("uright")
        elif kind == 4:    # radii: |dx| just below r, r = 0, r < 0, r NaN, a NaN centre
            d = f32(x - dn(f32(x - r)))
            for q in ((f32(x - d), y, d, xr, -1, -1), (x, y, f32(0), xr, -1, -1), (x, y, f32(-1), xr, -1, -1),
                      (x, y, f32(np.nan), xr, -1, -1), (f32(np.nan), y, r, xr, -1, -1)):
                qs.append(q); target.append(j); tags.append("radius")
        else:              # the cell range: the window reaches past the grid's edge
            qs.append((x, y, f32(700.0), xr, -1, -1)); target.append(j); tags.append("cells")
    q = np.array(qs, R.WQ_DTYPE)
    qdesc = desc[np.array(target)]
    return dict(kps=kps, desc=desc, uright=ur, bounds=BOUNDS, queries=q, qdesc=qdesc, target=np.array(target), tags=tags)


def nan_keypoints(seed=0, n=300):
    """Keypoints with NaN and +-inf coordinates among ordinary ones (PosInGrid: outside the grid on x86-64)."""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, R_KP)
    kps["x"] = rng.uniform(0, 640, n); kps["y"] = rng.uniform(0, 480, n); kps["octave"] = rng.integers(0, 8, n)
    bad = rng.choice(n, 40, replace=False)
    vals = [np.nan, np.inf, -np.inf, 1e10, -1e10]
    for k, j in enumerate(bad):
        kps["x" if k % 2 else "y"][j] = vals[k % len(vals)]
        if k % 7 == 0:
            kps["x"][j] = kps["y"][j] = np.nan
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return kps, desc


# ------------------------------------------------------------------------------------------------------------ rotation
def histogram_cases():
    """Bin sizes at ComputeThreeMaxima's 10 % rule: max2 (max3) = 0.1 max1 exactly and one either side."""
    cases = []
    for m1, m2, m3 in ((30, 3, 2), (30, 2, 1), (30, 4, 3), (30, 4, 2), (10, 1, 1), (10, 0, 0), (9, 1, 0), (31, 3, 3), (100, 10, 9),
                       (100, 10, 10), (100, 9, 9), (7, 7, 7), (1, 1, 1), (0, 0, 0), (50, 5, 4), (50, 6, 5)):
        h = np.zeros(R.HISTO_LENGTH, np.int32)
        h[[3, 17, 8]] = (m1, m2, m3)
        cases.append(h)
    return cases


def rotation_angles():
    """Angle pairs on the bin edges (rot * (1/30) = k + 0.5 and one ulp either side) and around the 360-degree wrap."""
    out = []
    fac = f32(f32(1) / f32(30))
    for k in range(12):
        t = f32(f32(k + 0.5) / fac)
        for rot in (t, np.nextafter(t, f32(0)), np.nextafter(t, f32(400))):
            out.append((f32(rot), f32(0)))
    for a2 in (f32(1e-3), np.nextafter(f32(0), f32(1)), f32(359.99997), f32(0.5)):
        out.append((f32(0), a2))
    out.append((f32(359.99997), f32(0))); out.append((f32(0), f32(0)))
    return out


def rotation_scene(counts=None, seed=0):
    """One query per lattice keypoint, centred on it with its descriptor: every query matches its keypoint.  counts = matches per
    rotation bin (e.g. {0: 31, 5: 3, 9: 2}: 3 < 0.1f * 31 drops bin 5); None = the angle pairs of rotation_angles(), on the bin edges."""
    w = window_scene(seed)
    kps = w["kps"].copy()
    pairs = [(f32(30 * b + 1), f32(0)) for b, c in sorted(counts.items()) for _ in range(c)] if counts else rotation_angles()
    n = len(pairs)
    assert n <= len(kps)
    kps = kps[:n].copy()
    kps["angle"] = [a2 for _, a2 in pairs]
    qangle = np.array([a1 for a1, _ in pairs], f32)
    q = np.zeros(n, R.WQ_DTYPE)
    q["u"], q["v"], q["r"], q["min_level"], q["max_level"] = kps["x"], kps["y"], f32(3.0), -1, -1
    return dict(kps=kps, desc=w["desc"][:n].copy(), bounds=BOUNDS, queries=q, qdesc=w["desc"][:n].copy(), qangle=qangle,
                takes=np.ones(n, np.uint8))


ROTATION_COUNTS = [{0: 31, 5: 3, 9: 2}, {0: 30, 5: 3, 9: 2}, {0: 30, 5: 4, 9: 3}, {2: 50, 7: 5, 11: 4}, {1: 19, 4: 2, 12: 1},
                   {0: 9, 6: 1}, {3: 10, 8: 1, 10: 1}]


def rotation_kept(sc):
    """The restated rotation check when every query matches its own keypoint: (bins, kept mask)."""
    bins = np.array([R.rot_bin(a1, a2) for a1, a2 in zip(sc["qangle"], sc["kps"]["angle"])])
    hist = np.bincount(bins, minlength=R.HISTO_LENGTH)
    keep = {i for i in R.three_maxima(hist) if i >= 0}
    return bins, np.isin(bins, sorted(keep))
