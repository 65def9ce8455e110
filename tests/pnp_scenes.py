"""Synthetic PnPsolver problems for tests/test_cpu_pnp.py and tests/test_gpu_pnp.py: a 640 x 480 pinhole camera at a planted pose,
points 2 to 10 units in front of it, octaves 0 to 7.  Planted inliers are noise-free (their float32 pixel is the projection of the
float32 point to rounding); planted outliers are displaced by at least 20 px (the threshold at octave 7 is about 8.8 px).  A
problem is a dict with the fields of orbm_pnp_problem (cam = fu, fv, uc, vc) plus the truth: R, t, inlier [n] bool.  The sets are
pre-drawn with the problem's seed."""
import numpy as np

NLEVELS = 8
SIGMA2 = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2          # mvLevelSigma2 of the default pyramid
CAM = (517.3, 516.5, 318.6, 255.3)
TH2 = 5.991


def rotation(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def draw_sets(rng, n, H, frame_rule=False):
    """the draw loop of PnPsolver.cc:193-206 (frame_rule: of :304-317) with rng.integers as RandomInt"""
    out = np.zeros((H, 4), np.int32)
    for h in range(H):
        avail, size = list(range(n)), n
        for i in range(4):
            r = int(rng.integers(0, size))
            idx = avail[r]
            out[h, i] = idx
            avail[idx if frame_rule else r] = avail[size - 1]
            size -= 1
    return out


def problem(seed, n, H, outliers=0.3, axis=(0.3, 1.0, -0.2), deg=25.0, t=(0.4, -0.3, 0.6), min_inliers=None, frame_rule=False, name=None):
    """n correspondences, H drawn sets; outliers: share of correspondences whose pixel is somewhere else (at least 20 px away)"""
    rng = np.random.default_rng(seed)
    R = rotation(axis, deg); t = np.asarray(t, np.float64)
    z = rng.uniform(2.0, 10.0, n)
    u = rng.uniform(20.0, 620.0, n); v = rng.uniform(20.0, 460.0, n)
    Xc = np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)
    Xw = ((Xc - t) @ R).astype(np.float32)                      # R^T (Xc - t)
    Xc = Xw.astype(np.float64) @ R.T + t                        # the pixel of the float32 point
    uv = np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)
    bad = rng.random(n) < outliers
    if n >= 8:
        bad[:8][rng.permutation(8)[:6]] = False                 # at least six planted inliers
    ang = rng.uniform(0, 2 * np.pi, n); r = rng.uniform(20.0, 120.0, n)
    uv[bad] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)[bad]
    if min_inliers is None:
        min_inliers = max(8, int(np.float32(n) * np.float32(0.4)), 4)
    return dict(name=name or f"n{n}_H{H}_seed{seed}", n=n, H=H, Xw=Xw, uv=uv.astype(np.float32), octave=rng.integers(0, NLEVELS, n).astype(np.int32),
                cam=CAM, th2=TH2, min_inliers=min_inliers, sets=draw_sets(rng, n, H, frame_rule) if n >= 4 else np.zeros((0, 4), np.int32),
                R=R, t=t, inlier=~bad)


def fold_scenes():
    """the scenes of the planted-mask assertions and of the folds: seeds whose drawn sets hold more than one record, so that
    speculative Refines (records behind the one that succeeds) are on the path"""
    return [problem(34, 60, 300, outliers=0.3, name="n60"),
            problem(33, 130, 300, outliers=0.45, deg=70.0, t=(-0.5, 0.2, 1.0), name="n130"),
            problem(32, 25, 300, outliers=0.2, axis=(1.0, 0.1, 0.4), deg=-40.0, name="n25")]


def degenerate_sets(prob, rng):
    """Xw, uv, octave of `prob` with eight rows appended that make degenerate minimal sets, and those sets [k][4]: a repeated
    index (twice, and all four the same), four coplanar points, four collinear points, a point at the camera centre, a NaN
    coordinate"""
    n = prob["n"]
    R, t = prob["R"], prob["t"]
    Xc = np.array([[0.5, 0.2, 4.0], [-0.4, 0.3, 4.0], [0.1, -0.6, 4.0], [0.7, 0.6, 4.0],          # coplanar in the camera frame (z = 4)
                   [-1.0, -0.5, 3.0], [0.0, 0.0, 5.0], [0.5, 0.25, 6.0], [1.0, 0.5, 7.0]])        # collinear
    Xw = ((Xc - t) @ R).astype(np.float32)
    Xcf = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([CAM[0] * Xcf[:, 0] / Xcf[:, 2] + CAM[2], CAM[1] * Xcf[:, 1] / Xcf[:, 2] + CAM[3]], 1).astype(np.float32)
    centre = (-(R.T @ t)).astype(np.float32)                     # the camera centre in the world
    nan = np.array([np.nan, 1.0, 2.0], np.float32)
    Xw = np.concatenate([prob["Xw"], Xw, centre[None], nan[None]]); uv = np.concatenate([prob["uv"], uv, [[300.0, 200.0]], [[100.0, 100.0]]]).astype(np.float32)
    octave = np.concatenate([prob["octave"], rng.integers(0, NLEVELS, 10).astype(np.int32)])
    sets = np.array([[0, 1, 1, 2], [3, 3, 3, 3], [5, 4, 5, 4], [n, n + 1, n + 2, n + 3], [n + 4, n + 5, n + 6, n + 7], [n + 8, 0, 1, 2],
                     [n + 9, 0, 1, 2], [0, 1, 2, n + 9]], np.int32)
    return Xw, uv, octave, sets
