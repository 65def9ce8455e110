"""Synthetic monocular initialisations for tests/test_cpu_init.py and tests/test_gpu_init.py: a 640 x 480 pinhole camera that sees
the same points from two poses, X2 = R X1 + t (so R, t are the R21, t21 the Initializer returns, t up to scale).  A scene is a dict:
keys1 [n1, 2], keys2 [n2, 2] (every keypoint of the two frames: Normalize sums over all of them, matched or not), matches12 [n1]
(index into keys2 or -1), matches [n, 2] (mvMatches12), sets [H, 8] pre-drawn as :82-97 draws them, K, and the truth: R, t, bad [n]
(the matches that were sent somewhere else), H21 for a planar scene."""
import numpy as np

W, HGT = 640, 480
K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]], np.float32)
PLANE_N, PLANE_D = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0]), 4.0     # n . X = d in camera 1


def rotation(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def draw_sets(rng, n, H):
    """the draw loop of Initializer.cc:82-97 with rng.integers as RandomInt"""
    out = np.zeros((H, 8), np.int32)
    for h in range(H):
        avail = list(range(n))
        for j in range(8):
            r = int(rng.integers(0, len(avail)))
            out[h, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def scene(seed, n, H, kind="general", noise=0.0, outliers=0.0, extra=5, axis=(0.2, 1.0, -0.1), deg=6.0, t=(1.0, 0.15, 0.1), name=None):
    """n matches, H drawn sets.  kind: "general" (depths 2 .. 8) or "planar" (the plane PLANE_N . X = PLANE_D).  noise: standard
    deviation in pixels added to both images; outliers: share of matches whose second keypoint is somewhere else; extra: unmatched
    keypoints in each frame."""
    rng = np.random.default_rng(seed)
    Kd = K.astype(np.float64)
    R, t = rotation(axis, deg), np.asarray(t, np.float64)
    n1, n2 = n + extra, n + extra
    px = np.stack([rng.uniform(20, W - 20, n1), rng.uniform(20, HGT - 20, n1)], 1)
    rays = np.concatenate([(px - Kd[:2, 2]) / [Kd[0, 0], Kd[1, 1]], np.ones((n1, 1))], 1)
    z = PLANE_D / (rays @ PLANE_N) if kind == "planar" else rng.uniform(2.0, 8.0, n1)
    X1 = rays * np.reshape(z, (-1, 1))
    X2 = X1 @ R.T + t
    p2 = (X2 / X2[:, 2:3]) @ Kd.T
    first = np.sort(rng.permutation(n1)[:n])                    # the matched keypoints of frame 1, ascending as mvMatches12 lists them
    second = rng.permutation(n2)[:n]                            # where each stands in frame 2
    keys2 = np.stack([rng.uniform(20, W - 20, n2), rng.uniform(20, HGT - 20, n2)], 1)
    keys2[second] = p2[first, :2]
    bad = rng.random(n) < outliers
    keys2[second[bad]] = np.stack([rng.uniform(20, W - 20, int(bad.sum())), rng.uniform(20, HGT - 20, int(bad.sum()))], 1)
    keys1 = px + rng.standard_normal((n1, 2)) * noise
    keys2 = keys2 + rng.standard_normal((n2, 2)) * noise
    matches12 = np.full(n1, -1, np.int32); matches12[first] = second
    out = dict(name=name or f"{kind}_n{n}_H{H}_seed{seed}", kind=kind, n=n, H=H, keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32),
               matches12=matches12, matches=np.stack([first, second], 1).astype(np.int32), sets=draw_sets(rng, n, H) if n >= 8 else np.zeros((0, 8), np.int32),
               K=K, R=R, t=t, bad=bad, X1=X1[first], sigma=1.0)
    if kind == "planar":
        out["H21"] = Kd @ (R + np.outer(t, PLANE_N) / PLANE_D) @ np.linalg.inv(Kd)
    return out


EDGE_N, EDGE_H = (8, 9, 63, 64, 65, 129), (1, 5, 200)
NOISE, OUTLIERS = 0.01, 0.05         # chosen so that the flags near a threshold stay under the cap (tests/test_cpu_init.py measures the share)


def edge_scenes():
    """n at the minimum set and at the wave and mask-word edges x H in {1, 5, 200}"""
    return [scene(200 + 10 * k + j, n, H, kind="planar" if (k + j) % 3 == 2 else "general", noise=NOISE, outliers=OUTLIERS if n > 9 else 0.0,
                  name=f"edge_n{n}_H{H}")
            for k, n in enumerate(EDGE_N) for j, H in enumerate(EDGE_H)]


def restatement_scenes():
    """the larger scenes of the device-against-restatement comparison"""
    return [scene(301, 300, 200, "general", NOISE, OUTLIERS, name="general_300"), scene(302, 300, 200, "planar", NOISE, OUTLIERS, name="planar_300"),
            scene(303, 150, 200, "general", 2 * NOISE, 2 * OUTLIERS, extra=40, name="general_150")]


def compared_scenes():
    """every scene tests/test_gpu_init.py holds against the restatement"""
    return edge_scenes() + restatement_scenes()


# ---- planted cases (tests/test_cpu_init.py on the restatement, tests/test_gpu_init.py through the device)
def singular_scene():
    """Integer pixel coordinates in pairs x, 640 - x, so that the mean of frame 1 is exactly x = 320; the matches 40 .. 47
    lie on that line, exactly collinear: their normalised u1 is 0, three columns of ComputeH21's A are zero, vt.row(8) is a unit
    vector, Hn has one non-zero entry, H21i two zero rows or a zero column -- a determinant of exactly 0 -- so H12i is all zero
    and every chiSquare is NaN"""
    rng = np.random.default_rng(13)
    s = scene(13, 40, 3, "planar")
    a = rng.integers(40, 300, 20).astype(np.float64)
    x = np.concatenate([a, 640 - a])                           # with the eight at 320 the sum over all 48 keypoints is 48 * 320
    k1 = np.concatenate([np.stack([x, rng.integers(40, 440, 40)], 1), np.stack([np.full(8, 320.0), 60.0 + 40 * np.arange(8)], 1)])
    q = np.c_[k1, np.ones(48)] @ s["H21"].T
    k2 = q[:, :2] / q[:, 2:]
    m = np.stack([np.arange(48), np.arange(48)], 1).astype(np.int32)
    sets = np.concatenate([np.arange(40, 48, dtype=np.int32)[None], s["sets"]])
    return dict(s, keys1=k1.astype(np.float32), keys2=k2.astype(np.float32), matches=m, matches12=np.arange(48, dtype=np.int32), sets=sets, n=48, H=4,
                name="singular")


def zero_score_scene():
    """sigma = 1e-5 makes every chiSquare of a noisy scene exceed its threshold: every score of both models is exactly 0"""
    return dict(scene(14, 60, 20, "general", noise=0.3), sigma=1e-5, name="zero_scores")


def rt_scene(depths, t=(0.2, 0.0, 0.0), deg=0.0, extra_unmatched=2):
    """points on distinct rays at the given depths (negative: behind both cameras), seen exactly by both cameras"""
    rng = np.random.default_rng(len(depths))
    n = len(depths)
    R, t = rotation((0, 1, 0), deg), np.asarray(t, np.float64)
    px = np.stack([rng.uniform(60, 580, n), rng.uniform(60, 420, n)], 1)
    X = np.c_[(px - [320, 240]) / 500.0, np.ones(n)] * np.asarray(depths, np.float64)[:, None]
    X2 = X @ R.T + t
    p2 = (X2 / X2[:, 2:]) @ K.astype(np.float64).T
    k1 = np.concatenate([px, rng.uniform(50, 400, (extra_unmatched, 2))]); k2 = np.concatenate([rng.uniform(50, 400, (extra_unmatched, 2)), p2[:, :2]])
    m = np.stack([np.arange(n), extra_unmatched + np.arange(n)], 1).astype(np.int32)
    return k1.astype(np.float32), k2.astype(np.float32), m, R, t, X
