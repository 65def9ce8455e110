"""The loops `for pKFi in targets: matcher.Fuse(pKFi, vpMapPoints)` of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:550-558)
and `matcher.Fuse(pKF, Scw, mvpLoopMapPoints, 4, vpReplacePoints)` + the Replace loop of LoopClosing::SearchAndFuse
(src/LoopClosing.cc:587-613), stated literally: per target oracle.project_points -> oracle.search_fuse with the list's descriptors
AS THEY ARE AT THAT MOMENT -> the loop tail, on a toy map of several keyframes (ToyWorld) that restates what the loops can observe
of the KeyFrame / MapPoint pointer graph.  CPU only; nothing of the package under test is used here.

ToyWorld restates
  MapPoint::AddObservation            src/MapPoint.cc:113-132  (nObs += 2 for a stereo keypoint)
  KeyFrame::AddMapPoint               src/KeyFrame.cc:221-233  (mvpMapPoints[idx] = pMP)
  KeyFrame::EraseMapPointMatch / ReplaceMapPointMatch          (:241-253, :269-272)
  KeyFrame::GetMapPoints              :274-287                 (the slots' non-NULL, non-bad points)
  MapPoint::Replace                   src/MapPoint.cc:240-278  (with its IsInKeyFrame branch and the closing
                                                                ComputeDistinctiveDescriptors on the heir, :275)
  MapPoint::ComputeDistinctiveDescriptors  :305-370            (through oracle.distinctive_descriptors)
  MapPoint::IsInKeyFrame (:387-391) / Observations (:203-207) / isBad (:280-285).
mObservations is a std::map<KeyFrame*, size_t>, iterated in pointer order; here a keyframe's id stands for its address: the
observations of a point are visited in ascending keyframe id (this fixes the order of the rows ComputeDistinctiveDescriptors
compares, hence which descriptor wins a tie of medians)."""
import copy

import numpy as np

import oracle

TH_LOW = 45                                     # src/ORBmatcher.cc:37


class ToyKeyFrame:
    def __init__(self, kfid, desc, uright):
        self.id = kfid
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.uright = np.ascontiguousarray(uright, np.float32)        # mvuRight (-1: monocular keypoint)
        self.slots = np.full(len(self.desc), -1, np.int64)            # mvpMapPoints: handle or -1


class ToyWorld:
    """keyframes by id, map points by handle 0 .. n-1; every mutation the loops perform is logged in self.ops."""

    def __init__(self, npoints):
        self.kfs = {}
        self.bad = np.zeros(npoints, bool)
        self.nobs = np.zeros(npoints, np.int64)                       # nObs
        self.obs = [dict() for _ in range(npoints)]                   # mObservations: keyframe id -> keypoint index
        self.desc = np.zeros((npoints, 32), np.uint8)                 # mDescriptor
        self.ops = []
        self.heir_events = []                                         # (handle) of every Replace's heir, in order

    def clone(self):
        return copy.deepcopy(self)

    def add_keyframe(self, kfid, desc, uright):
        self.kfs[kfid] = ToyKeyFrame(kfid, desc, uright)
        return self.kfs[kfid]

    # ---- MapPoint
    def is_in_keyframe(self, h, kfid):
        return kfid in self.obs[h]

    def add_observation(self, h, kfid, idx):                           # MapPoint.cc:113-132
        if kfid in self.obs[h]:
            return
        self.obs[h][kfid] = int(idx)
        self.nobs[h] += 2 if self.kfs[kfid].uright[idx] >= 0 else 1

    def compute_distinctive_descriptors(self, h):                      # MapPoint.cc:305-370 (no keyframe of the toy map is bad)
        if self.bad[h] or not self.obs[h]:
            return
        rows = np.stack([self.kfs[k].desc[i] for k, i in sorted(self.obs[h].items())])
        best = oracle.distinctive_descriptors(rows, np.array([0, len(rows)], np.int32))[0]
        self.desc[h] = rows[best]

    def replace(self, dead, heir):                                     # MapPoint.cc:240-278: dead->Replace(heir)
        if dead == heir:
            return
        obs = self.obs[dead]
        self.obs[dead] = {}
        self.bad[dead] = True
        for kfid, idx in sorted(obs.items()):
            kf = self.kfs[kfid]
            if not self.is_in_keyframe(heir, kfid):
                kf.slots[idx] = heir                                   # ReplaceMapPointMatch
                self.add_observation(heir, kfid, idx)
            else:
                kf.slots[idx] = -1                                     # EraseMapPointMatch
        self.compute_distinctive_descriptors(heir)
        self.heir_events.append(int(heir))

    # ---- KeyFrame
    def add_map_point(self, kfid, h, idx):                             # KeyFrame.cc:221-233
        self.kfs[kfid].slots[idx] = h

    def get_map_points(self, kfid):                                    # KeyFrame.cc:274-287
        s = self.kfs[kfid].slots
        return {int(h) for h in s if h >= 0 and not self.bad[h]}

    def state(self):
        """everything a later reader of the map could see"""
        return (self.bad.copy(), self.nobs.copy(), [sorted(o.items()) for o in self.obs], self.desc.copy(),
                {k: kf.slots.copy() for k, kf in self.kfs.items()})


def same_state(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and
            a[4].keys() == b[4].keys() and all(np.array_equal(a[4][k], b[4][k]) for k in a[4]))


def candidate_rows(scene, targets, points, desc, active, sim3):
    """oracle.project_points -> oracle.search_fuse per target over the list entries `points` with the descriptors `desc`; an
    inactive pair has the presets 256, -1, visible 0.  Returns (best, idx, visible), each [len(targets)][len(points)]."""
    pts = np.asarray(points, np.int64)
    best = np.full((len(targets), len(pts)), 256, np.int32); idx = np.full((len(targets), len(pts)), -1, np.int32)
    vis = np.zeros((len(targets), len(pts)), np.int32)
    for r, t in enumerate(targets):
        proj, q = oracle.project_points(2 if sim3 else 1, scene.pos[pts], scene.nrm[pts], scene.mind[pts], scene.maxd[pts], t.R, t.t, t.Ow,
                                        scene.cam4, t.bounds, t.mbf, 0.5, scene.logsf, scene.sf, scene.th)
        b, ix = oracle.search_fuse(q, desc, t.kps, t.desc, t.bounds, t.uright, None if sim3 else scene.inv_sigma2)
        on = np.ones(len(pts), bool) if active is None else np.asarray(active[r]) != 0
        best[r, on], idx[r, on], vis[r, on] = b[on], ix[on], proj["visible"][on]
    return best, idx, vis


def literal_loop(scene, world, sim3=False, freeze_descriptors=False):
    """The sequential loop on `world` (changed in place).  Returns (nFused per target, refreshes, changed) -- refreshes = the number
    of targets k < K - 1 after which the descriptor of some non-bad list entry is not the bytes the rows of target k were computed
    with; changed = how many of those moved an entry of a LATER target's (best, idx) row.  freeze_descriptors: the candidate rows
    keep using the descriptors of the loop's start (what a replay of the first call's rows WITHOUT refresh does)."""
    lst, K = scene.lst, len(scene.targets)
    li = np.maximum(lst, 0)
    start = world.desc[li].copy()
    used = start.copy()                          # per entry: the bytes a one-call-plus-refresh scheme would hold (for the two counts only)
    nFused, refreshes, changed = [], 0, 0
    everything = np.arange(len(lst))
    for k, t in enumerate(scene.targets):
        now = start if freeze_descriptors else world.desc[li]        # pMP->GetDescriptor() of every entry, read as target k begins
        best, idx, vis = (a[0] for a in candidate_rows(scene, [t], everything, now, None, sim3))
        n = 0
        if not sim3:                             # ORBmatcher.cc:1043-1172
            for i, h in enumerate(lst):
                if h < 0:                                                                   # :1047
                    continue
                if world.bad[h] or world.is_in_keyframe(h, t.id):                           # :1050
                    continue
                if not vis[i] or idx[i] < 0:                                                # :1057-1092, vIndices.empty()
                    continue
                if best[i] <= TH_LOW:                                                       # :1149
                    o = int(world.kfs[t.id].slots[idx[i]])                                  # pKF->GetMapPoint(bestIdx)
                    if o >= 0:
                        if not world.bad[o]:
                            if world.nobs[o] > world.nobs[h]:
                                world.ops.append(("replace", k, int(h), o)); world.replace(h, o)     # :1157
                            else:
                                world.ops.append(("replace", k, o, int(h))); world.replace(o, h)     # :1159
                    else:
                        world.ops.append(("add", k, int(h), int(idx[i])))
                        world.add_observation(h, t.id, idx[i]); world.add_map_point(t.id, h, idx[i])    # :1164-1165
                    n += 1
        else:                                    # ORBmatcher.cc:1178-1301 and LoopClosing.cc:598-611
            already = world.get_map_points(t.id)                                            # :1194
            rep = np.full(len(lst), -1, np.int64)                                           # vpReplacePoints
            for i, h in enumerate(lst):
                if h < 0 or world.bad[h] or int(h) in already:                              # :1203 (NULL entries: the caller's list has none
                    continue                                                                 #  in the reference; here they are skipped)
                if not vis[i] or idx[i] < 0:
                    continue
                if best[i] <= TH_LOW:                                                       # :1279
                    o = int(world.kfs[t.id].slots[idx[i]])
                    if o >= 0:
                        if not world.bad[o]:
                            world.ops.append(("record", k, i, o)); rep[i] = o              # :1286
                    else:
                        world.ops.append(("add", k, int(h), int(idx[i])))
                        world.add_observation(h, t.id, idx[i]); world.add_map_point(t.id, h, idx[i])    # :1290-1291
                    n += 1
            for i, h in enumerate(lst):                                                     # LoopClosing.cc:604-611
                if rep[i] >= 0:
                    world.ops.append(("caller_replace", k, int(rep[i]), int(h))); world.replace(int(rep[i]), int(h))
        nFused.append(n)
        if k + 1 < K and not freeze_descriptors:
            now = world.desc[li]
            live = (lst >= 0) & ~world.bad[li]
            moved = live & (now != used).any(axis=1)
            if moved.any():
                refreshes += 1
                later = scene.targets[k + 1:]
                b0, i0, _ = candidate_rows(scene, later, everything[moved], used[moved], None, sim3)
                b1, i1, _ = candidate_rows(scene, later, everything[moved], now[moved], None, sim3)
                changed += int(not (np.array_equal(b0, b1) and np.array_equal(i0, i1)))
                used[moved] = now[moved]
    return nFused, refreshes, changed


class WorldOps:
    """ToyWorld behind the map_ops interface of ORBmatcher.fuse_keyframes (the handles are the toy map's), logging what the literal
    loop logs."""

    def __init__(self, scene, world, sim3=False):
        self.s, self.w, self.sim3, self.k = scene, world, sim3, -1

    def _kf(self): return self.s.targets[self.k].id
    def is_bad(self, h): return bool(self.w.bad[h])
    def is_in_keyframe(self, h): return self.w.is_in_keyframe(h, self._kf())
    def slot_owner(self, idx): return int(self.w.kfs[self._kf()].slots[idx])
    def observations(self, h): return int(self.w.nobs[h])
    def descriptor(self, h): return self.w.desc[h].tobytes()

    def in_target(self, h, k):
        kf = self.s.targets[k].id
        return int(h) in self.w.get_map_points(kf) if self.sim3 else self.w.is_in_keyframe(h, kf)

    def replace(self, dead, heir):
        self.w.ops.append(("replace", self.k, int(dead), int(heir))); self.w.replace(dead, heir)

    def add(self, h, idx):
        self.w.ops.append(("add", self.k, int(h), int(idx)))
        self.w.add_observation(h, self._kf(), idx); self.w.add_map_point(self._kf(), h, idx)

    def begin_target(self, k):
        self.k = k
        if self.sim3:
            self.already = self.w.get_map_points(self._kf())
            self.rep = {}

    def already_found(self, h): return int(h) in self.already

    def record_replace(self, i, h):
        self.w.ops.append(("record", self.k, int(i), int(h))); self.rep[int(i)] = int(h)

    def end_target(self, k, report):
        if not self.sim3:
            return
        for i in sorted(self.rep):                                       # LoopClosing.cc:604-611
            h = int(self.s.lst[i])
            self.w.ops.append(("caller_replace", k, self.rep[i], h)); self.w.replace(self.rep[i], h)
            report(i)
