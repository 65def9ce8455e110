"""Scenes for the tests of the Fuse loop over several target keyframes (tests/test_cpu_fuse_keyframes.py,
tests/test_gpu_fuse_keyframes.py): a list of map points, K target keyframes with poses, keypoints and slot owners, and the toy map
of tests/fuse_keyframes_reference.py behind them.  The map-point arrays are indexed by LIST position, as ORBmatcher.Fuse takes them.
  flip_scene()     (a) the hand-made case: a Replace at target 0 changes the list entry's distinctive descriptor, and a keypoint of
                   target 1 that was out of reach comes within TH_LOW;
  random_scene()   (b) seeded: duplicates and NULL entries in the list, stereo and mono keypoints, owners with more and with fewer
                   observations, bad points, points already in a target."""
import numpy as np

import oracle
from fuse_keyframes_reference import ToyWorld
from orb_slam2_e_amd.extractor import KP_DTYPE

CAM4 = np.array([718.856, 718.856, 607.19, 185.22], np.float32)
BOUNDS = (0.0, 0.0, 1241.0, 376.0)
MBF = 386.1448
SF = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))]).astype(np.float32)).astype(np.float32)
LOGSF = np.float32(np.log(np.float32(1.2)))                    # mfLogScaleFactor = log(mfScaleFactor)
INV_SIGMA2 = (1.0 / (SF * SF)).astype(np.float32)
NOISE = 0.08         # bit-flip rate of an observation against its point: two observations differ by about 38 bits, so TH_LOW (45) cuts through


def cam_record(bounds=BOUNDS):
    from orb_slam2_e_amd.matcher import ORBmatcher
    cam = np.zeros(1, ORBmatcher.CAM_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"] = CAM4
    cam["gminx"], cam["gminy"], cam["gmaxx"], cam["gmaxy"] = bounds
    cam["min_x"], cam["min_y"], cam["max_x"], cam["max_y"] = (int(b) for b in bounds)
    return cam


class Target:
    """one target keyframe: id, pose (Rcw, tcw, Ow as float32), keypoints, descriptors, mvuRight (None: monocular keyframe)"""

    def __init__(self, kfid, R, t, kps, desc, uright, bounds=BOUNDS, mbf=MBF):
        self.id = kfid
        self.R = np.ascontiguousarray(R, np.float32).reshape(3, 3); self.t = np.ascontiguousarray(t, np.float32).reshape(3)
        self.Ow = (-(self.R.T @ self.t)).astype(np.float32)
        self.kps, self.desc, self.uright, self.bounds, self.mbf = kps, np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), uright, bounds, mbf
        self._dev = None

    def device(self):
        """the orbm_fuse_target of this keyframe (the frame is made resident once)"""
        from orb_slam2_e_amd import Frame, FuseTarget
        if self._dev is None:
            self._dev = FuseTarget(Frame(self.kps, self.desc, self.bounds, self.uright), self.R, self.t, self.Ow, cam_record(self.bounds), self.mbf)
        return self._dev


class Scene:
    cam4, sf, logsf, inv_sigma2 = CAM4, SF, LOGSF, INV_SIGMA2

    def __init__(self, lst, pos, nrm, mind, maxd, targets, world, th):
        self.lst = np.ascontiguousarray(lst, np.int32)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        self.pos, self.nrm, self.mind, self.maxd = f32(pos), f32(nrm), f32(mind), f32(maxd)
        self.targets, self.world, self.th = targets, world, float(th)

    def list_descriptors(self, world=None):
        """GetDescriptor() of every list entry (zeros for a NULL entry)"""
        d = (world or self.world).desc[np.maximum(self.lst, 0)].copy()
        d[self.lst < 0] = 0
        return d


def flip(d, bits):
    out = np.array(d, np.uint8).copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def noisy(rng, d, p):
    return d ^ np.packbits(rng.random(256) < p, bitorder="little")


def _kps(xy, octave):
    k = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, np.float32).T
    k["octave"] = octave
    return k


def _pose(rng, amount):
    from scipy.spatial.transform import Rotation
    R = Rotation.from_euler("xyz", rng.uniform(-0.04, 0.04, 3) * amount).as_matrix().astype(np.float32)
    return R, (rng.uniform(-0.3, 0.3, 3) * amount).astype(np.float32)


def _cloud(rng, n):
    """points in front of a camera near the origin: positions, normals (towards the camera, perturbed), distance ranges"""
    z = rng.uniform(4, 14, n)
    u = rng.uniform(-60, 1300, n); v = rng.uniform(-30, 400, n)
    pos = np.stack([(u - CAM4[2]) * z / CAM4[0], (v - CAM4[3]) * z / CAM4[1], z], 1).astype(np.float32)
    nrm = pos / np.linalg.norm(pos, axis=1, keepdims=True) + rng.normal(0, 0.35, (n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    d = np.linalg.norm(pos, axis=1)
    maxd = (d * rng.uniform(0.95, 3.7, n)).astype(np.float32)
    mind = (maxd / rng.uniform(3.9, 4.6, n)).astype(np.float32)
    return pos, nrm, mind, maxd


def project(t, pos, nrm, mind, maxd, th, sim3):
    return oracle.project_points(2 if sim3 else 1, pos, nrm, mind, maxd, t.R, t.t, t.Ow, CAM4, t.bounds, t.mbf, 0.5, LOGSF, SF, th)


def flip_scene():
    """(a): list = [P].  P has two observations (descriptors A1, A2; its distinctive descriptor is A1).  Target 0 has a keypoint at
    P's projection with descriptor B1 (40 bits from A1: within TH_LOW), owned by O, whose two observations B1, B2 are 4 bits apart:
    Observations(O) == Observations(P), so O->Replace(P), and P's distinctive descriptor over {A1, B1, A2, B2} is B1.  Target 1 has a
    free keypoint at P's projection with descriptor C: 70 bits from A1 (out of reach), 30 from B1."""
    rng = np.random.default_rng(5)
    A1 = rng.integers(0, 256, 32, dtype=np.uint8)
    B1 = flip(A1, range(0, 40)); B2 = flip(B1, range(40, 44)); A2 = flip(A1, range(100, 130)); Cd = flip(B1, range(200, 230))
    pos = np.array([[0.4, -0.2, 8.0]], np.float32); nrm = np.array([[0.0, 0.0, 1.0]], np.float32)
    mind = np.array([3.0], np.float32); maxd = np.array([12.0], np.float32)
    th = 3.0
    targets = []
    for k, (kfid, d) in enumerate(((10, B1), (20, Cd))):
        R, t = _pose(rng, 1.0)
        tg = Target(kfid, R, t, _kps(np.zeros((0, 2)), 0), np.zeros((0, 32), np.uint8), None)
        proj, _ = project(tg, pos, nrm, mind, maxd, th, False)
        assert proj["visible"][0]
        far = rng.integers(0, 256, (3, 32), dtype=np.uint8)             # three more keypoints elsewhere in the image
        xy = np.array([[proj["u"][0], proj["v"][0]], [100, 100], [900, 300], [600, 50]], np.float32)
        targets.append(Target(kfid, R, t, _kps(xy, int(proj["level"][0])), np.concatenate([d[None], far]), None))
    w = ToyWorld(2)
    for tg in targets:
        w.add_keyframe(tg.id, tg.desc, np.full(len(tg.desc), -1, np.float32))
    for kfid, d in ((5, A1), (15, A2), (25, B2)):
        w.add_keyframe(kfid, d[None], np.array([-1], np.float32))
    P, O = 0, 1
    w.add_observation(P, 5, 0); w.add_observation(P, 15, 0)
    w.add_observation(O, 10, 0); w.add_map_point(10, O, 0); w.add_observation(O, 25, 0)
    w.compute_distinctive_descriptors(P); w.compute_distinctive_descriptors(O)
    assert np.array_equal(w.desc[P], A1)
    return Scene([P], pos, nrm, mind, maxd, targets, w, th)


def random_scene(seed, K=4, U=260, sim3=False, nclutter=120, ndup=32, nnull=6, mono_last=True):
    """(b): U distinct list points (+ duplicates and NULL entries), K targets around one cloud.  Every point has 1-3 observations in
    keyframes outside the loop (noisy copies of its own descriptor); a target sees a keypoint near most of the projections that
    fall into it, again a noisy copy, free or owned by another map point with 1-5 observations, by a bad one, or by the list point
    itself.  The last target is monocular (mvuRight NULL) when mono_last, the others mix stereo and mono keypoints."""
    rng = np.random.default_rng(seed)
    th = 4.0 if sim3 else 3.0
    P, N, mind, maxd = _cloud(rng, U)
    true = rng.integers(0, 256, (U, 32), dtype=np.uint8)
    extra_ids = [10 * j + 5 for j in range(6)]
    extra_rows = {e: [] for e in extra_ids}
    obs = []                                     # (handle, keyframe id, keypoint index), keyframes filled below
    owners_of = []                               # descriptor cluster of every owner handle U, U + 1, ...

    def outside_observations(h, cluster, count):
        for e in rng.choice(extra_ids, count, replace=False):
            extra_rows[int(e)].append(noisy(rng, true[cluster], NOISE)); obs.append((h, int(e), len(extra_rows[int(e)]) - 1))

    for h in range(U):
        outside_observations(h, h, int(rng.integers(1, 4)))
    targets, slots, bad_owners = [], [], []
    for k in range(K):
        R, t = _pose(rng, 1.0 if k else 0.0)
        probe = Target(10 * (k + 1), R, t, None, np.zeros((0, 32), np.uint8), None)
        proj, _ = project(probe, P, N, mind, maxd, th, sim3)
        xy, octv, desc, ur, own = [], [], [], [], []
        mono = mono_last and k == K - 1
        for h in np.nonzero(proj["visible"])[0]:
            if rng.random() > 0.8:
                continue
            xy.append((proj["u"][h] + rng.normal(0, 0.4), proj["v"][h] + rng.normal(0, 0.4)))
            octv.append(max(int(proj["level"][h]) - int(rng.integers(0, 2)), 0))
            desc.append(noisy(rng, true[h], NOISE))
            ur.append(-1.0 if mono or rng.random() < 0.5 else proj["ur"][h] + rng.normal(0, 0.3))
            c = rng.random()
            if c < 0.45:                         # owned by another map point of the same descriptor cluster
                o = U + len(owners_of); owners_of.append(h); own.append(o)
                if rng.random() < 0.08:
                    bad_owners.append(o)
            elif c < 0.52:
                own.append(int(h))               # the list point is already in this keyframe
            else:
                own.append(-1)
        for _ in range(nclutter):
            xy.append((rng.uniform(0, 1241), rng.uniform(0, 376))); octv.append(int(rng.integers(0, 8)))
            desc.append(rng.integers(0, 256, 32, dtype=np.uint8)); ur.append(-1.0 if mono or rng.random() < 0.5 else xy[-1][0] - rng.uniform(0, 40))
            own.append(-1)
        targets.append(Target(probe.id, R, t, _kps(np.array(xy, np.float32), np.array(octv)), np.array(desc, np.uint8),
                              None if mono else np.array(ur, np.float32)))
        slots.append(own)
    w = ToyWorld(U + len(owners_of))
    for o, cluster in enumerate(owners_of):
        outside_observations(U + o, cluster, int(rng.integers(0, 4)))
    for tg in targets:
        w.add_keyframe(tg.id, tg.desc, tg.uright if tg.uright is not None else np.full(len(tg.desc), -1, np.float32))
    for e in extra_ids:
        rows = np.array(extra_rows[e], np.uint8).reshape(-1, 32)
        w.add_keyframe(e, rows, np.full(len(rows), -1, np.float32))
    for h, kfid, idx in obs:
        w.add_observation(h, kfid, idx)
    for tg, own in zip(targets, slots):
        seen = set()
        for idx, h in enumerate(own):
            if h < 0 or h in seen:               # a point observes a keyframe once
                continue
            seen.add(h)
            w.add_observation(h, tg.id, idx); w.add_map_point(tg.id, h, idx)
    for h in range(len(w.bad)):
        w.compute_distinctive_descriptors(h)
    w.bad[bad_owners] = True
    w.bad[rng.choice(U, max(U // 30, 1), replace=False)] = True          # a few list points are bad from the start
    lst = np.concatenate([rng.permutation(U), rng.integers(0, U, ndup), np.full(nnull, -1)]).astype(np.int32)
    rng.shuffle(lst)
    li = np.maximum(lst, 0)
    return Scene(lst, P[li], N[li], mind[li], maxd[li], targets, w, th)
