"""Synthetic frames for Optimizer::PoseOptimization: keypoints with map points seen from a known camera pose, pixel noise per
octave, stereo right coordinates on part of them, injected gross outliers, optional points at z = 0 or behind the camera, and a
start pose some degrees / centimetres away from the truth."""
import numpy as np

CAM = (517.306408, 516.469215, 318.643040, 255.313989, 40.0)      # fx fy cx cy mbf (TUM1-like pinhole, 0.077 m baseline)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-15:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose44(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def inv_level_sigma2(nlevels=8, scale=1.2):
    return (1.0 / (scale ** np.arange(nlevels)) ** 2).astype(np.float32)


def make_problem(seed, n, stereo_frac=0.0, outlier_frac=0.0, noise_px=0.5, rot_deg=3.0, trans_m=0.05, fill=0.85, z0=0, behind=0,
                 nlevels=8, scale=1.2):
    """n keypoints, about fill * n of them with a map point, on an nlevels pyramid of the given scale (pixel noise noise_px *
    scale^octave, inv_sigma2 to match).  Returns a dict: kp_xy[n,2], octave[n], uright[n] (-1: mono), has_mp[n], mp_pos[n,3],
    cam, inv_sigma2, Tcw (the start pose), Ttrue."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = CAM
    Rt = rodrigues(rng.normal(0, 0.3, 3)); tt = rng.normal(0, 0.5, 3)
    Pc = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n), np.ones(n)], 1) * rng.uniform(1.0, 8.0, (n, 1))
    idx = rng.permutation(n)
    for k in idx[:z0]:
        Pc[k, 2] = 0.0                                  # z = 0 at the true pose
    for k in idx[z0:z0 + behind]:
        Pc[k, 2] = -Pc[k, 2]                            # behind the camera
    Xw = ((Pc - tt) @ Rt).astype(np.float32)            # world = Rt^T (Pc - tt)
    Pc = Xw.astype(np.float64) @ Rt.T + tt
    octave = rng.integers(0, nlevels, n).astype(np.int32)
    sig = scale ** octave
    with np.errstate(divide="ignore", invalid="ignore"):
        u = Pc[:, 0] / Pc[:, 2] * fx + cx
        v = Pc[:, 1] / Pc[:, 2] * fy + cy
        ur = u - bf / Pc[:, 2]
    u = np.where(np.isfinite(u), u, rng.uniform(0, 640, n)) + rng.normal(0, noise_px, n) * sig
    v = np.where(np.isfinite(v), v, rng.uniform(0, 480, n)) + rng.normal(0, noise_px, n) * sig
    ur = np.where(np.isfinite(ur), ur, u - 5) + rng.normal(0, noise_px, n) * sig
    bad = rng.random(n) < outlier_frac
    u[bad] += rng.choice([-1, 1], bad.sum()) * rng.uniform(20, 80, bad.sum())
    v[bad] += rng.choice([-1, 1], bad.sum()) * rng.uniform(20, 80, bad.sum())
    stereo = (rng.random(n) < stereo_frac) & (Pc[:, 2] > 0)
    uright = np.where(stereo, ur, -1.0).astype(np.float32)
    has_mp = (rng.random(n) < fill).astype(np.uint8)
    has_mp[idx[:z0 + behind]] = 1
    R0 = rodrigues(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rot_deg)) @ Rt
    t0 = tt + rng.normal(0, trans_m / np.sqrt(3), 3)
    kp_xy = np.stack([u, v], 1).astype(np.float32)
    return {"kp_xy": kp_xy, "octave": octave, "uright": uright, "has_mp": has_mp, "mp_pos": Xw, "cam": np.array(CAM, np.float32),
            "inv_sigma2": inv_level_sigma2(nlevels, scale), "Tcw": pose44(R0, t0), "Ttrue": pose44(Rt, tt), "Rt": Rt, "tt": tt,
            "bad": bad & (has_mp > 0)}


def noise_free(seed, n, stereo, rot_deg=4.0, trans_m=0.06):
    """A noise-free scene on which every quantity is exact: camera (512, 512, 320, 240, bf 32), true rotation 90 degrees about z,
    dyadic translation, camera-frame points with power-of-two depth and dyadic x / y, so Xw, the observations and the
    projections at the true pose are exact floats and the optimum is the true pose itself."""
    rng = np.random.default_rng(seed)
    cam = np.array([512.0, 512.0, 320.0, 240.0, 32.0], np.float32)
    Rt = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tt = np.array([0.25, -0.125, 0.5])
    z = 2.0 ** rng.integers(0, 4, n)
    Pc = np.stack([rng.integers(-150, 151, n) / 256 * z, rng.integers(-110, 111, n) / 256 * z, z], 1)
    Xw = ((Pc - tt) @ Rt).astype(np.float32)
    assert np.array_equal(Xw.astype(np.float64) @ Rt.T + tt, Pc)
    u = Pc[:, 0] / Pc[:, 2] * 512 + 320
    v = Pc[:, 1] / Pc[:, 2] * 512 + 240
    ur = (u - 32 / Pc[:, 2]) if stereo else -np.ones(n)
    R0 = rodrigues(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rot_deg)) @ Rt
    t0 = tt + rng.normal(0, trans_m / np.sqrt(3), 3)
    return {"kp_xy": np.stack([u, v], 1).astype(np.float32), "octave": rng.integers(0, 8, n).astype(np.int32),
            "uright": ur.astype(np.float32), "has_mp": np.ones(n, np.uint8), "mp_pos": Xw, "cam": cam,
            "inv_sigma2": inv_level_sigma2(8), "Tcw": pose44(R0, t0), "Ttrue": pose44(Rt, tt), "Rt": Rt, "tt": tt,
            "bad": np.zeros(n, bool)}
