"""Stereo pairs for Frame::ComputeStereoMatches at its edges (src/Frame.cc:527-701), shared by the CPU and the GPU tests and
tests/fuzz_fem_stereo.py.  Numpy only, seeded: identical wherever they are generated.

A scene is a dict: name, prm (nFeatures, scaleFactor, nLevels, iniThFAST, minThFAST), mb, mbf (float32, maxD = mbf / mb),
left, right (uint8 h x w) and, for integer shifts, d (right(x) = left(x + d): a left point at uL is at uL - d on the right).
"""
import numpy as np

from orb_slam2_e_amd.synth import _scene, synth_stereo_pair

f32 = np.float32

# the reference's stereo settings (Examples/Stereo/*.yaml; roslaunch/sHamlyn01.yaml for the fork's pyramid)
KITTI00 = dict(prm=(2000, 1.2, 8, 20, 7), fx=718.856, bf=386.1448)     # KITTI00-02.yaml:8,25,38-51
KITTI03 = dict(prm=(2000, 1.2, 8, 20, 7), fx=721.5377, bf=387.5744)    # KITTI03.yaml:8,25,38-51; 1241 x 376 (:18-19)
KITTI04 = dict(prm=(2000, 1.2, 8, 12, 7), fx=707.0912, bf=379.8145)    # KITTI04-12.yaml:8,25,38-51 (iniThFAST 12, :50)
EUROC = dict(prm=(1200, 1.2, 8, 20, 7), fx=435.2047, bf=47.9064)       # EuRoC.yaml:8,25,88-101; 752 x 480 (:18-19)
FORK = dict(prm=(1200, 1.1, 6, 24, 7), fx=381.670013, bf=40.0)         # sHamlyn01.yaml:9,71-84 (the file has no bf: 40 chosen)


def _mk(name, s, left, right, d=None, mb=None):
    mbf = f32(s["bf"])
    return dict(name=name, prm=s["prm"], mb=f32(mb) if mb is not None else f32(mbf / f32(s["fx"])), mbf=mbf,
                left=np.ascontiguousarray(left), right=np.ascontiguousarray(right), d=d)


def texture(seed, w, h, density=1.0):
    """synth_frame's statistics (rectangles, discs, noise) on any canvas."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    a = w * h / (640 * 480) * density
    img = _scene(rng, w, h, max(1, int(300 * a)), max(1, int(200 * a))) + rng.integers(-6, 7, size=(h, w), dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def shifted(seed, w, h, d):
    """right(x) = left(x + d) for an integer d (d < 0: the right content lies to the right)."""
    c = texture(seed, w + abs(d), h)
    return (c[:, :w], c[:, d:d + w]) if d >= 0 else (c[:, -d:-d + w], c[:, :w])


def photometric(img, seed, gain=1.0, offset=0.0, noise=0.0, blur=0):
    rng = np.random.default_rng(seed)
    x = img.astype(np.float64) * gain + offset
    if blur:
        k = np.ones(2 * blur + 1) / (2 * blur + 1)
        x = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, x)
    x += rng.normal(0, noise, x.shape) if noise else 0
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def subpixel(seed, w, h, dmin, dmax):
    left, right = synth_stereo_pair(seed, w=w, h=h, dmin=dmin, dmax=dmax)
    return left, right


# ------------------------------------------------------------------------------------------------------------- settings
def kitti03(seed=0):
    return _mk("kitti03", KITTI03, *subpixel(seed, 1241, 376, 2.0, 60.0))


def kitti04(seed=1):
    return _mk("kitti04", KITTI04, *subpixel(seed, 1241, 376, 2.0, 60.0))


def euroc_near_maxd(seed=2):
    """EuRoC (maxD = fx ~ 435 px) with the right image shifted by 430 px: just below maxD."""
    l, r = shifted(seed, 752, 480, 430)
    return _mk("euroc_d430", EUROC, l, r, d=430)


def fork_pyramid(seed=3):
    return _mk("fork_1.1x6", FORK, *subpixel(seed, 640, 480, 1.0, 30.0))


def one_level(seed=4):
    s = dict(KITTI00, prm=(1000, 1.2, 1, 20, 7))
    return _mk("nlevels1", s, *subpixel(seed, 640, 480, 2.0, 40.0))


def coarse_pyramid(seed=5):
    s = dict(KITTI00, prm=(1000, 1.5, 4, 20, 7))
    return _mk("scale1.5x4", s, *subpixel(seed, 640, 480, 2.0, 40.0))


# ------------------------------------------------------------------------------------------------------------- disparity
def shift(d, seed=6, w=640, h=480, setting=KITTI00, mb=None, name=None):
    l, r = shifted(seed, w, h, d)
    return _mk(name or f"shift{d}", setting, l, r, d=d, mb=mb)


def small_maxd(seed=7, d=30.0):
    """mbf / mb = 384 / 16 = 24 px exactly: a sub-pixel field of 18-30 px straddles maxD (the range gate and the range reject),
    and level-0 right keypoints lie exactly on minU = uL - 24."""
    l, r = subpixel(seed, 640, 480, 18.0, d)
    return _mk("maxD24", dict(KITTI00, bf=384.0), l, r, mb=16.0)


# ------------------------------------------------------------------------------------------------------------- photometric
def photometric_right(seed=8):
    """Gain, offset, noise and a blur on the right image: L1 minima at the window's edge, flat parabolas, a wide SAD spread."""
    l, r = subpixel(seed, 640, 480, 2.0, 40.0)
    r = photometric(r, seed, gain=0.8, offset=20, noise=6.0, blur=1)
    return _mk("photometric", KITTI00, l, r)


def half_identical(seed=9, d=12):
    """Right = left shifted by d with noise, except a block where right == left: zero disparities clamped to 0.01 with an L1
    distance of 0, below the noisy half's median, so the clamp survives the cut."""
    l, r = shifted(seed, 640, 480, d)
    l = l.copy(); r = photometric(r, seed, noise=4.0)
    # the identical block is noise-free rectangles: a step edge moved one pixel either way costs the same L1, so d1 == d3,
    # deltaR == 0 and the disparity is exactly 0
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    l[120:360, 160:480] = r[120:360, 160:480] = np.clip(_scene(rng, 320, 240, 60, 0), 0, 255).astype(np.uint8)
    return _mk("half_identical", KITTI00, l, r)


# ------------------------------------------------------------------------------------------------------------- geometry
def tall(seed=11, d=9):
    """2080 x 4000: nRows next to the 4,096 rows of the device row table.  (The level's FAST area must keep an aspect ratio of
    at least 0.5 -- one initial octree node, ORBextractor.cc:543 -- which 2000 x 4000 misses by the borders.)"""
    l, r = shifted(seed, 2080, 4000, d)
    return _mk("tall_2080x4000", dict(KITTI00, prm=(2000, 1.2, 8, 20, 7)), l, r, d=d)


def dense_band(seed=12, d=7):
    """5000 features from about 30 textured rows: row lists far longer than 128 (the device scans a row 64 lanes at a time)."""
    l, r = shifted(seed, 1241, 376, d)
    l = l.copy(); r = r.copy()
    rng = np.random.default_rng(seed)
    band = rng.integers(0, 256, (30, 1241 + d), dtype=np.uint8)
    for img, off in ((l, 0), (r, d)):
        img[:, :] = 128
        img[170:200] = band[:, off:off + 1241]
    return _mk("dense_band", dict(KITTI00, prm=(5000, 1.2, 8, 20, 7)), l, r, d=d)


# ------------------------------------------------------------------------------------------------------------- counts
def flat_left(seed=13):
    l, r = shifted(seed, 640, 480, 5)
    return _mk("flat_left", KITTI00, np.full_like(l, 128), r)


def flat_right(seed=14):
    l, r = shifted(seed, 640, 480, 5)
    return _mk("flat_right", KITTI00, l, np.full_like(r, 128))


def unrelated_noise(seed=15):
    """Two independent images of uniform noise: descriptors about 128 bits apart, none below 70, nd = 0."""
    rng = np.random.default_rng(seed)
    return _mk("unrelated_noise", KITTI00, rng.integers(0, 256, (480, 640), dtype=np.uint8), rng.integers(0, 256, (480, 640), dtype=np.uint8))


def batch_scenes():
    """Six 640 x 480 pairs of one setting, ragged in every count: N = 0, no candidates, nd = 0 and three that match."""
    return [flat_left(), flat_right(), unrelated_noise(), shift(1, seed=16), half_identical(), photometric_right()]


def edge_scenes():
    """The single-pair scenes (the batch and the tall frame apart)."""
    return [kitti03(), kitti04(), euroc_near_maxd(), fork_pyramid(), one_level(), coarse_pyramid(),
            shift(0), shift(1), shift(-8, name="wrong_way"), small_maxd(), photometric_right(), half_identical(),
            dense_band()]


def random_scene(rng):
    """A fuzz case: one of the generators above with random seeds, or a random setting on a sub-pixel pair."""
    k = int(rng.integers(0, 8))
    seed = int(rng.integers(0, 1 << 20))
    if k == 0:
        return shift(int(rng.integers(-20, 60)), seed=seed)
    if k == 1:
        return small_maxd(seed, d=float(rng.uniform(20, 40)))
    if k == 2:
        return photometric_right(seed)
    if k == 3:
        return half_identical(seed, d=int(rng.integers(1, 40)))
    s = dict(KITTI00, prm=(int(rng.integers(50, 2500)), float(rng.choice([1.1, 1.2, 1.3, 1.5, 2.0])), int(rng.integers(1, 9)),
                           int(rng.integers(8, 30)), int(rng.integers(3, 9))),
             fx=float(rng.uniform(300, 900)), bf=float(rng.uniform(20, 500)))
    w, h = int(rng.integers(400, 1300)), int(rng.integers(240, 500))
    return _mk("random", s, *subpixel(seed, w, h, float(rng.uniform(0, 5)), float(rng.uniform(10, 90))))
