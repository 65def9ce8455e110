"""Synthetic refinement attempts of LoopClosing::ComputeSim3 (src/LoopClosing.cc:311-341) for tests/test_cpu_refine_sim3.py and
tests/test_gpu_refine_sim3.py: a FAMILY is one current keyframe KF1 of map 1 and the points it observes; an ATTEMPT is a candidate
keyframe KF2 of map 2 that observes some of the same 3-D points, map 2 being map 1 under a planted similarity (Xc1 = s R Xc2 + t, as
tests/sim3_opt_scenes.py), plus the start (R12, t12, s12) and the seeds the attempt begins with.  The attempts of a family share KF1,
as the attempts of one pass of the loop at LoopClosing.cc:288 do.

The start is the truth turned by `off_deg` about the axis tests/sim3_opt_scenes.py uses, translation and scale `off` too large.  The
attempts that live on their seeds start 5 degrees / 5 % off, as there.  At 520 px of focal length 5 degrees are 45 px, six times the
7.5-px window of SearchBySim3 at level 0: from there the search finds nothing (the shape "seeds only").  The attempts whose shape
needs the search to find pairs start 0.2 degrees / 0.2 % off, which is what Sim3Solver hands over in the reference (its inliers
reproject within sqrt(9.21) sigma).

A map point's distance bounds are set so that PredictScale gives its partner keypoint's octave in the other keyframe (ratio =
0.9 sf[octave]: the 5 % of the far start move log(ratio) / log(1.2) by 0.27 of a level, not across one)."""
import functools

import numpy as np

from orb_slam2_e_amd.extractor import KP_DTYPE
from sim3_scenes import pose, rotation

NLEVELS = 8
SF = np.ones(NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    SF[_i] = np.float32(SF[_i - 1] * np.float32(1.2))
LOG_SF = np.float32(np.log(np.float32(1.2)))
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)
CAM = np.array([520.0, 520.0, 320.0, 240.0], np.float32)
BOUNDS = (0.0, 0.0, 640.0, 480.0)
TH, TH_HIGH, TH2 = 7.5, 95, 10.0
FAR, NEAR = (5.0, 0.05), (0.2, 0.002)                      # (off_deg, off) of a start
T1W = pose((0.2, 1.0, 0.1), 25.0, (0.5, -0.1, 0.3))
T2W = pose((-0.3, 0.4, 1.0), -15.0, (-0.2, 0.3, 0.1))


def _project(X):
    return np.stack([CAM[0] * X[:, 0] / X[:, 2] + CAM[2], CAM[1] * X[:, 1] / X[:, 2] + CAM[3]], 1)


def _to_world(T, Xc):
    return (Xc - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)


def _keypoints(xy, octave, rng):
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], octave
    k["angle"] = rng.uniform(0, 360, len(xy)); k["size"] = 31.0
    return k


def _observe(desc, rng, flip=0.03):
    return desc ^ np.packbits(rng.random((len(desc), 256)) < flip, axis=1, bitorder="little")


@functools.lru_cache(None)
def family(seed, n1, fix_scale=False, spread=1.0, p_valid=0.9):
    """KF1 with n1 keypoints, each with a map point (a share 1 - p_valid of them bad), and the points' images in map 2; spread
    narrows the field the points fill, so that KF2's image holds more of them"""
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else 1.7
    R = rotation((1.0, 2.0, -0.5), 10.0); t = np.array([0.3, -0.2, 0.4])
    z = rng.uniform(2.0, 8.0, n1)
    Xc1 = np.stack([rng.uniform(-0.5, 0.5, n1) * spread * z, rng.uniform(-0.38, 0.38, n1) * spread * z, z], 1)
    Xc2 = (Xc1 - t) @ R / s
    uv2 = _project(Xc2)
    seen2 = (Xc2[:, 2] > 0.2) & (uv2[:, 0] > 8) & (uv2[:, 0] < 632) & (uv2[:, 1] > 8) & (uv2[:, 1] < 472)
    oct1, oct2 = rng.integers(0, NLEVELS, n1), rng.integers(0, NLEVELS, n1)
    mp_desc = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    kps1 = _keypoints(_project(Xc1) + rng.standard_normal((n1, 2)), oct1, rng)
    maxd1 = (0.9 * np.linalg.norm(Xc2, axis=1) * SF[oct2]).astype(np.float32)     # KF1's points are searched for in KF2 ...
    maxd2 = (0.9 * np.linalg.norm(Xc1, axis=1) * SF[oct1]).astype(np.float32)     # ... and KF2's in KF1
    valid1 = (rng.random(n1) < p_valid).astype(np.uint8)
    return dict(seed=seed, n1=n1, fix_scale=int(fix_scale), s=s, R=R, t=t, Xc1=Xc1, Xc2=Xc2, uv2=uv2, seen2=seen2, oct2=oct2, mp_desc=mp_desc,
                kps1=kps1, desc1=_observe(mp_desc, rng), valid1=valid1, pos1=_to_world(T1W, Xc1).astype(np.float32),
                mind1=(maxd1 / SF[-1]).astype(np.float32), maxd1=maxd1, maxd2=maxd2)


def attempt(fam, name, seed, shared, clutter=20, start=NEAR, seeds=0.0, minus2=0, onto_invalid=0, blocking=0, outliers=0.0, wrong_seeds=0,
            p_valid2=0.92, noise=1.0):
    """KF2 observes `shared` of the family's points (those its image holds, at most) plus `clutter` keypoints of its own.
    seeds: the share of the common pairs the attempt starts from (the solver's inliers).  minus2: that many more KF1 slots seeded
    with -2.  onto_invalid: that many seeds whose KF2 map point is bad.  blocking: that many seeds that name the KF2 keypoint ANOTHER
    KF1 point would have matched.  outliers: share of KF2's shared keypoints moved 15 .. 60 px.  wrong_seeds: seeds onto clutter."""
    rng = np.random.default_rng(seed)
    n1 = fam["n1"]
    pool = np.nonzero(fam["seen2"])[0]
    pts = np.sort(rng.choice(pool, min(shared, len(pool)), replace=False))          # family points KF2 observes
    m = len(pts)
    n2 = m + clutter
    order = rng.permutation(n2)                                                      # keypoint j of KF2 shows entry order[j]
    xy = np.concatenate([fam["uv2"][pts] + noise * rng.standard_normal((m, 2)), np.stack([rng.uniform(10, 630, clutter), rng.uniform(10, 470, clutter)], 1)])
    bad = rng.random(m) < outliers
    xy[:m][bad] += rng.choice([-1.0, 1.0], (int(bad.sum()), 2)) * rng.uniform(15.0, 60.0, (int(bad.sum()), 2))
    octave = np.concatenate([fam["oct2"][pts], rng.integers(0, NLEVELS, clutter)])
    zc = rng.uniform(2.0, 8.0, clutter)
    Xc2 = np.concatenate([fam["Xc2"][pts], np.stack([(xy[m:, 0] - CAM[2]) / CAM[0] * zc, (xy[m:, 1] - CAM[3]) / CAM[1] * zc, zc], 1)])
    mp_desc = np.concatenate([fam["mp_desc"][pts], rng.integers(0, 256, (clutter, 32), dtype=np.uint8)])
    maxd = np.concatenate([fam["maxd2"][pts], (0.9 * np.linalg.norm(Xc2[m:], axis=1) * SF[octave[m:]]).astype(np.float32)])
    valid2 = (rng.random(n2) < p_valid2).astype(np.uint8)
    e = lambda a: np.ascontiguousarray(a[order])
    where = np.empty(n2, np.int64); where[order] = np.arange(n2)                    # entry -> keypoint of KF2
    partner = np.full(n1, -1, np.int64); partner[pts] = where[:m]                   # KF1 keypoint -> the KF2 keypoint of the same point
    valid2 = e(valid2)
    seed12 = np.full(n1, -1, np.int32)
    good = pts[(fam["valid1"][pts] == 1) & (valid2[partner[pts]] == 1)]
    for i1 in rng.permutation(good)[:int(round(seeds * len(good)))]:
        seed12[i1] = partner[i1]
    free = [int(i) for i in rng.permutation(good) if seed12[i] == -1]
    for _ in range(minus2):
        seed12[free.pop()] = -2
    inval = [int(i) for i in pts if fam["valid1"][i] == 1 and valid2[partner[i]] == 0]
    for i1 in inval[:onto_invalid]:
        seed12[i1] = partner[i1]
    for _ in range(blocking):                                                        # a's seed takes b's partner: b finds nothing
        a, b = free.pop(), free.pop()
        seed12[a] = partner[b]
    unseen = [int(i) for i in range(n1) if fam["valid1"][i] == 1 and partner[i] < 0]
    own = [int(where[m + k]) for k in range(clutter) if valid2[where[m + k]] == 1]
    for k in range(wrong_seeds):                                                     # a KF1 point KF2 does not see, onto a keypoint of KF2's own
        seed12[unseen[k]] = own[k]
    off_deg, off = start
    R0 = fam["R"] @ rotation((0.3, -1.0, 0.6), off_deg)
    return dict(name=name, family=fam, n2=n2, kps2=_keypoints(e(xy), e(octave), rng), desc2=_observe(e(mp_desc), rng), valid2=valid2,
                pos2=e(_to_world(T2W, Xc2).astype(np.float32)), maxd2=e(maxd), mind2=(e(maxd) / SF[-1]).astype(np.float32), mp_desc2=e(mp_desc),
                seed12=seed12, partner=partner, R12=R0.astype(np.float32), t12=(fam["t"] * (1 + off)).astype(np.float32),
                s12=np.float32(fam["s"] if fam["fix_scale"] else fam["s"] * (1 + off)), T2w=T2W, shape=name.split("@")[0])


def empty_attempt(fam, name="n2_zero"):
    """a candidate without keypoints"""
    z = lambda *s: np.zeros(s, np.float32)
    return dict(name=name, family=fam, n2=0, kps2=np.zeros(0, KP_DTYPE), desc2=np.zeros((0, 32), np.uint8), valid2=np.zeros(0, np.uint8),
                pos2=z(0, 3), maxd2=z(0), mind2=z(0), mp_desc2=np.zeros((0, 32), np.uint8), seed12=np.full(fam["n1"], -1, np.int32),
                partner=np.full(fam["n1"], -1, np.int64), R12=fam["R"].astype(np.float32), t12=fam["t"].astype(np.float32),
                s12=np.float32(fam["s"]), T2w=T2W, shape=name)


N1, N1_BIG = 220, 620
SMALL = {   # shape: keyword arguments of attempt()
    "seeds_only": dict(shared=150, start=FAR, seeds=0.6, outliers=0.1),
    "search_only": dict(shared=170, clutter=30),
    "both": dict(shared=180, seeds=0.3, outliers=0.05),
    "minus2": dict(shared=160, seeds=0.3, minus2=6),
    "seed_invalid2": dict(shared=160, seeds=0.3, onto_invalid=4),
    "seed_blocks": dict(shared=160, seeds=0.3, blocking=3),
    "few": dict(shared=12, clutter=140, start=FAR, seeds=1.0, wrong_seeds=4),
    "none": dict(shared=0, clutter=150),
}
# (attempt seed, pixel noise in KF2) per (shape, scale fixed).  OptimizeSim3 stops a round only after three iterations that each gain
# less than 0.1 %, so a well-conditioned scene spends its last iterations at the rounding floor, where the sign of rho -- hence the
# iteration and trial counts -- is decided by the last bits of chi2 (tests/sim3_opt_scenes.py).  The seeds are the first from 1 on
# for which the RESTATEMENT alone (never the device) passes the selection rule of tests/test_cpu_sim3_opt.py: no chi2 of a cut
# within M D th2 of th2, no trial with |rho| below 1e-9, the same integers under all 16 patterns of the +-1 ulp switch.
# tests/test_cpu_refine_sim3.py holds every scene to it.
SEEDS = {("seeds_only", False): (1, 1.0), ("search_only", False): (22, 1.0), ("both", False): (3, 1.0), ("minus2", False): (9, 1.0),
         ("seed_invalid2", False): (5, 1.0), ("seed_blocks", False): (4, 1.0), ("few", False): (1, 1.0), ("none", False): (1, 1.0),
         ("seeds_only", True): (6, 1.0), ("search_only", True): (72, 1.0), ("both", True): (33, 1.0), ("minus2", True): (9, 1.0),
         ("seed_invalid2", True): (9, 1.0), ("seed_blocks", True): (6, 1.0), ("few", True): (2, 1.0), ("none", True): (1, 1.0)}
BIG_SEED = (7, 1.0)
FAMILY_SEED = {False: 1, True: 2, "big": 3}


def fam(fix_scale=False):
    return family(FAMILY_SEED[fix_scale], N1, fix_scale)


@functools.lru_cache(None)
def small(name, fix_scale=False):
    seed, noise = SEEDS[(name, fix_scale)]
    return attempt(fam(fix_scale), f"{name}@{'fixed' if fix_scale else 'free'}", seed, noise=noise, **SMALL[name])


@functools.lru_cache(None)
def big():
    """about 600 keypoints and more than 512 correspondences: the pairs behind SO_LDS_PAIRS take k_sim3_optimize's far path"""
    return attempt(family(FAMILY_SEED["big"], N1_BIG, spread=0.55, p_valid=0.97), "big@free", BIG_SEED[0], shared=N1_BIG, clutter=10, seeds=0.9,
                   outliers=0.05, p_valid2=0.97, noise=BIG_SEED[1])


def batches():
    """name -> (fix_scale, [attempts]): every small shape alone with the scale free and fixed, the candidate without keypoints, the
    big scene, a ragged batch of three with different n2, and 64 attempts made of repeats of the small ones"""
    out = {}
    for fixed in (False, True):
        for name in SMALL:
            a = small(name, fixed)
            out[a["name"]] = (fixed, [a])
    out["n2_zero"] = (False, [empty_attempt(fam())])
    out["big"] = (False, [big()])
    out["ragged3"] = (False, [small("both"), small("few"), small("search_only")])
    names = list(SMALL)
    out["p64"] = (False, [small(names[k % len(names)]) if k % 9 != 8 else empty_attempt(fam()) for k in range(64)])
    return out
