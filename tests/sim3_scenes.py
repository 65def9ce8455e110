"""Synthetic Sim3Solver problems for tests/test_cpu_sim3.py and tests/test_gpu_sim3.py: two keyframes of two maps that see the same
points, map 2 being map 1 under a similarity (the drift a loop closure corrects).  A problem is a dict with the fields of
orbm_sim3_problem (cam1 / cam2 = fx, fy, cx, cy) plus the truth: s, R, t with Xc1 = s R Xc2 + t."""
import numpy as np

NLEVELS = 8
SIGMA2 = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2          # mvLevelSigma2 of the default pyramid
CAM1 = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
CAM2 = np.array([480.0, 490.0, 315.0, 236.0], np.float32)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, deg); T[:3, 3] = t
    return T.astype(np.float32)


def draw_triples(rng, n, H):
    """the draw loop of Sim3Solver.cc:163-177 with rng.integers as RandomInt"""
    out = np.zeros((H, 3), np.int32)
    for h in range(H):
        avail = list(range(n))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def problem(seed, n, H, s=1.7, axis=(1.0, 2.0, -0.5), deg=40.0, t=(0.3, -0.2, 0.4), noise=0.0, outliers=0.0, fix_scale=False, name=None):
    """n correspondences, H drawn triples.  noise: standard deviation of the second map's points, in units of depth / fx (pixels);
    outliers: share of correspondences whose second point is somewhere else."""
    rng = np.random.default_rng(seed)
    if fix_scale:
        s = 1.0
    R = rotation(axis, deg); t = np.asarray(t, np.float64)
    z = rng.uniform(2.0, 8.0, n)
    Xc1 = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    Xc2 = (Xc1 - t) @ R / s                                     # R^T (Xc1 - t) / s
    Xc2 += rng.standard_normal((n, 3)) * (noise * np.abs(Xc2[:, 2:3]) / 480.0)
    bad = rng.random(n) < outliers
    Xc2[bad] += rng.uniform(-1.0, 1.0, (int(bad.sum()), 3))
    Tcw1 = pose((0.2, 1.0, 0.1), 25.0, (0.5, -0.1, 0.3)); Tcw2 = pose((-0.3, 0.4, 1.0), -15.0, (-0.2, 0.3, 0.1))
    to_world = lambda T, Xc: (Xc - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)
    return dict(name=name or f"n{n}_H{H}_seed{seed}", n=n, H=H, fix_scale=int(fix_scale), X1w=to_world(Tcw1, Xc1).astype(np.float32),
                X2w=to_world(Tcw2, Xc2).astype(np.float32), octave1=rng.integers(0, NLEVELS, n).astype(np.int32),
                octave2=rng.integers(0, NLEVELS, n).astype(np.int32), Tcw1=Tcw1, Tcw2=Tcw2, cam1=CAM1, cam2=CAM2,
                triples=draw_triples(rng, n, H) if n >= 3 else np.zeros((0, 3), np.int32), s=s, R=R, t=t, bad=bad)


def restatement_scenes():
    """the scenes of the cap check and of the device-against-restatement comparison"""
    return [problem(11, 100, 300, noise=1.0, outliers=0.3, name="n100"),
            problem(12, 1000, 300, noise=1.0, outliers=0.3, name="n1000"),
            problem(13, 129, 300, noise=2.0, outliers=0.5, fix_scale=True, name="n129_fixed_scale"),
            problem(14, 40, 300, noise=3.0, outliers=0.2, deg=5.0, s=0.8, name="n40_small_rotation"),
            problem(15, 65, 150, noise=0.5, outliers=0.0, deg=170.0, name="n65_half_turn")]
