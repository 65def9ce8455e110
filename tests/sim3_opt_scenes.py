"""Synthetic OptimizeSim3 problems for tests/test_cpu_sim3_opt.py and tests/test_gpu_sim3_opt.py, built like tests/sim3_scenes.py: two
keyframes of two maps that see the same points, map 2 being map 1 under a similarity, pixel noise on both keyframes' observations
and a share of gross outliers.  A problem is a dict with the fields of orbm_sim3_opt_problem (cam1 / cam2 = fx, fy, cx, cy) plus
the truth: s, R, t with Xc1 = s R Xc2 + t.  The start (R12, t12, s12) is the truth turned by `off_deg` about a fixed axis, with the
translation and the scale `off` too large, in float as LoopClosing.cc:320-325 hands it over."""
import numpy as np

from sim3_scenes import CAM1, CAM2, NLEVELS, SIGMA2, pose, rotation

INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)                         # mvInvLevelSigma2
TH2 = 10.0                                                                          # LoopClosing.cc:329
SHAPES = (0, 1, 9, 10, 11, 63, 64, 65, 257, 300)


def problem(seed, n, s=1.7, axis=(1.0, 2.0, -0.5), deg=40.0, t=(0.3, -0.2, 0.4), noise=1.0, outliers=0.1, fix_scale=False, off_deg=5.0, off=0.05,
            th2=TH2, name=None):
    rng = np.random.default_rng(seed)
    if fix_scale:
        s = 1.0
    R = rotation(axis, deg); t = np.asarray(t, np.float64)
    z = rng.uniform(2.0, 8.0, n)
    Xc1 = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], 1)
    Xc2 = (Xc1 - t) @ R / s                                     # R^T (Xc1 - t) / s
    proj = lambda X, cam: np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], 1)
    obs1 = proj(Xc1, CAM1.astype(np.float64)) + noise * rng.standard_normal((n, 2))
    obs2 = proj(Xc2, CAM2.astype(np.float64)) + noise * rng.standard_normal((n, 2))
    bad = rng.random(n) < outliers
    k = int(bad.sum())
    obs2[bad] += rng.choice([-1.0, 1.0], (k, 2)) * rng.uniform(15.0, 60.0, (k, 2))
    Tcw1 = pose((0.2, 1.0, 0.1), 25.0, (0.5, -0.1, 0.3)); Tcw2 = pose((-0.3, 0.4, 1.0), -15.0, (-0.2, 0.3, 0.1))
    to_world = lambda T, Xc: (Xc - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)
    R0 = R @ rotation((0.3, -1.0, 0.6), off_deg)
    return dict(name=name or f"n{n}_seed{seed}{'_fixed' if fix_scale else ''}", n=n, fix_scale=int(fix_scale),
                X1w=to_world(Tcw1, Xc1).astype(np.float32), X2w=to_world(Tcw2, Xc2).astype(np.float32), obs1=obs1.astype(np.float32),
                obs2=obs2.astype(np.float32), octave1=rng.integers(0, NLEVELS, n).astype(np.int32),
                octave2=rng.integers(0, NLEVELS, n).astype(np.int32), Tcw1=Tcw1, Tcw2=Tcw2, cam1=CAM1, cam2=CAM2,
                R12=R0.astype(np.float32), t12=(t * (1 + off)).astype(np.float32), s12=np.float32(s if fix_scale else s * (1 + off)),
                th2=np.float32(th2), s=s, R=R, t=t, bad=bad)


# (seed, pixel noise, outlier share) per (n, scale fixed).  OptimizeSim3 stops a round only after three iterations that each gain
# less than 0.1 % (or at its iteration limit), so a well-conditioned scene spends its last iterations at the rounding floor, where
# the sign of rho -- accept or reject, hence the iteration and trial counts -- is decided by the last bits of chi2.  The seeds are
# the first from 200 on for which the RESTATEMENT (never the device) keeps every trial's |rho| above 1e-6 and every chi2 of a cut
# farther than 1e-4 th2 from th2, and gives the same integers under all 16 patterns of its +-1 ulp switch
# (tests/test_cpu_sim3_opt.py holds them to that); with the scale fixed that needed 1.5 px of noise.  n = 10 with the scale fixed has
# no such seed that reaches the second round: its scene stands on the other side of the < 10 rule (two pairs cut, 8 left).
SEEDS = {(0, False): (200, 1.0, 0.1), (0, True): (200, 1.0, 0.1), (1, False): (200, 1.0, 0.0), (1, True): (200, 1.0, 0.0),
         (9, False): (200, 1.0, 0.0), (9, True): (200, 1.0, 0.0), (10, False): (203, 1.0, 0.0), (10, True): (200, 1.0, 0.2),
         (11, False): (200, 1.0, 0.0), (11, True): (219, 1.5, 0.0), (63, False): (202, 1.0, 0.1), (63, True): (236, 1.5, 0.1),
         (64, False): (200, 1.0, 0.1), (64, True): (206, 1.5, 0.1), (65, False): (200, 1.0, 0.1), (65, True): (216, 1.5, 0.1),
         (257, False): (200, 1.0, 0.1), (257, True): (212, 1.5, 0.1), (300, False): (200, 1.0, 0.1), (300, True): (212, 1.5, 0.1)}


def gpu_scenes():
    """the scenes of the device-against-restatement comparison and of the sensitivity pass: every shape with the scale free and
    fixed, and the problem at the size limit"""
    out = []
    for n in SHAPES:
        for fixed in (False, True):
            seed, noise, outliers = SEEDS[(n, fixed)]
            out.append(problem(seed, n, fix_scale=fixed, noise=noise, outliers=outliers))
    out.append(problem(150, 8192, name="n8192"))
    return out


def nan_position(seed=31, n=40):
    """a pair whose map point of keyframe 1 is NaN: every sum it enters is NaN, no step is accepted, nothing is cut"""
    p = problem(seed, n, outliers=0.0, name="nan_position")
    p["X1w"][7] = np.nan
    return p


def all_outliers(seed=32, n=30):
    p = problem(seed, n, outliers=1.0, name="all_outliers")
    return p


def exact(n=60, fix_scale=False, moved=(7, 27, 47), off_deg=3.0, off=0.03):
    """the scene of tests/cxx/sim3_opt_smoke.cpp: both poses the identity, observations that are the exact projections of the
    float points, the pairs in `moved` shifted 40 px in keyframe 2, the start off_deg / off away"""
    s = 1.0 if fix_scale else 1.7
    R = rotation((1.0, 2.0, -0.5), 40.0); t = np.array([0.3, -0.2, 0.4])
    i = np.arange(n)
    z = 2.0 + 6.0 * ((i * 37) % 101) / 101.0
    X1 = np.stack([(((i * 53) % 97) / 97.0 - 0.5) * z, (((i * 29) % 89) / 89.0 - 0.5) * 0.8 * z, z], 1)
    X1w, X2w = X1.astype(np.float32), ((X1 - t) @ R / s).astype(np.float32)
    a, b = X1w.astype(np.float64), X2w.astype(np.float64)
    obs1 = np.stack([500 * a[:, 0] / a[:, 2] + 320, 500 * a[:, 1] / a[:, 2] + 240], 1).astype(np.float32)
    obs2 = np.stack([480 * b[:, 0] / b[:, 2] + 315, 490 * b[:, 1] / b[:, 2] + 236], 1).astype(np.float32)
    obs2[list(moved), 0] += 40
    bad = np.zeros(n, bool); bad[list(moved)] = True
    return dict(name=f"exact_n{n}{'_fixed' if fix_scale else ''}_{len(moved)}moved", n=n, fix_scale=int(fix_scale), X1w=X1w, X2w=X2w, obs1=obs1,
                obs2=obs2, octave1=(i % 8).astype(np.int32), octave2=((i + 3) % 8).astype(np.int32), Tcw1=np.eye(4, dtype=np.float32),
                Tcw2=np.eye(4, dtype=np.float32), cam1=np.float32([500, 500, 320, 240]), cam2=np.float32([480, 490, 315, 236]),
                R12=(R @ rotation((0.6, 0.0, 0.8), off_deg)).astype(np.float32), t12=((1 + off) * t).astype(np.float32),
                s12=np.float32(s if fix_scale else (1 + off) * s), th2=np.float32(TH2), s=s, R=R, t=t, bad=bad)
