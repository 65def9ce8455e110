#!/usr/bin/env python3
"""Call time of ORBmatcher::Fuse against K target keyframes (the forward loop of LocalMapping::SearchInNeighbors) on resident
2000-keypoint keyframes with a list of m = 2000 map points:
  (a) one call of orbm_fuse_keyframes over the K x m pairs (--masked F: with a mask that leaves a share F of the pairs inactive);
  (b) K x (orbm_project_points + orbm_frame_search_fuse) from this build;
  (c) with --parent-lib PATH (a build of the parent commit's library): the same K x two calls from that build, in the same process
      and the same alternation -- this change moves the projection arithmetic (b) runs into a shared device function.
K = 1, 5, 10, 20, 40, 100.  All forms go through bare ctypes with preallocated rows, so they differ in the library calls alone.
The forms alternate in one process; a figure is the median over batches of the mean of 10 calls, with the spread (min .. max over
batches) beside it.  Prints one JSON line per K.
--loop K: the whole loop instead (ORBmatcher.fuse_keyframes: mask, one call, replay, refreshes) on a scene of
tests/fuse_keyframes_scenes.random_scene with 2000 distinct list points, through the Python host logic and the toy map of the tests
(so its host share is Python's, not the C++ header's): the loop's time, its refreshes and waits, and the time of the same loop with
one project_points + frame_search_fuse + replay per target (the parent's path, which needs no refresh).

Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python tools/fuse_keyframes_time.py --batches 3` in a run of its own
and read k_fuse_keyframes against k_project_points + k_win_best from the statistics."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuse_keyframes_reference as R                                # noqa: E402
import fuse_keyframes_scenes as S                                   # noqa: E402
from orb_slam2_e_amd import ORBmatcher                              # noqa: E402
from orb_slam2_e_amd._lib import SO_PATH, lib, prototypes, ptr as _p   # noqa: E402
from orb_slam2_e_amd.matcher import _CCamera, _CFuseTarget          # noqa: E402

TH = 3.0


def timing_scene(K, m, nkp, seed=1):
    """m points, K targets of nkp keypoints each: a keypoint near the projection of most points a target sees (a noisy copy of the
    point's descriptor, stereo or mono), the rest clutter"""
    rng = np.random.default_rng(seed)
    P, N, mind, maxd = S._cloud(rng, m)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    targets = []
    for k in range(K):
        Rk, tk = S._pose(rng, 1.0 if k else 0.0)
        probe = S.Target(10 * (k + 1), Rk, tk, None, np.zeros((0, 32), np.uint8), None)
        proj, _ = S.project(probe, P, N, mind, maxd, TH, False)
        seen = np.nonzero(proj["visible"])[0]
        seen = seen[rng.random(len(seen)) < 0.8][:nkp]
        n1 = len(seen)
        xy = np.concatenate([np.stack([proj["u"][seen], proj["v"][seen]], 1) + rng.normal(0, 0.4, (n1, 2)),
                             np.stack([rng.uniform(0, 1241, nkp - n1), rng.uniform(0, 376, nkp - n1)], 1)]).astype(np.float32)
        octv = np.concatenate([np.maximum(proj["level"][seen] - rng.integers(0, 2, n1), 0), rng.integers(0, 8, nkp - n1)])
        noise = np.packbits(rng.random((n1, 256)) < 0.06, axis=1, bitorder="little")
        d = np.concatenate([desc[seen] ^ noise, rng.integers(0, 256, (nkp - n1, 32), dtype=np.uint8)])
        ur = np.where(rng.random(nkp) < 0.5, -1.0, xy[:, 0] - rng.uniform(0, 40, nkp)).astype(np.float32)
        ur[:n1] = np.where(ur[:n1] >= 0, proj["ur"][seen] + rng.normal(0, 0.3, n1), -1.0)
        targets.append(S.Target(probe.id, Rk, tk, S._kps(xy, octv), d, ur))
    return P, N, mind, maxd, desc, targets


class Build:
    """One build of the library through bare ctypes, outputs preallocated."""

    def __init__(self, path):
        self.L = lib() if path == SO_PATH else C.CDLL(path)
        for name in ("orbm_frame_create", "orbm_frame_destroy", "orbm_project_points", "orbm_frame_search_fuse", "orbm_fuse_keyframes"):
            if hasattr(self.L, name):
                fn = getattr(self.L, name)
                fn.restype, fn.argtypes = prototypes()[name]
        self.frames = []

    def prepare(self, P, N, mind, maxd, desc, targets, active):
        K, m = len(targets), len(P)
        self.K, self.m = K, m
        self.keep = (P, N, mind, maxd, desc, active)
        self.cam = S.cam_record()
        self.arr = (_CFuseTarget * K)()
        self.poses = []
        for c, t in zip(self.arr, targets):
            h = C.c_void_p()
            assert self.L.orbm_frame_create(_p(t.kps), _p(t.desc), len(t.kps), _p(t.uright), *S.BOUNDS, C.byref(h)) == 0
            self.frames.append(h)
            c.frame = h.value
            c.Rcw[:], c.tcw[:], c.Ow[:] = t.R.ravel().tolist(), t.t.tolist(), t.Ow.tolist()
            c.cam = _CCamera.from_buffer_copy(self.cam.tobytes()); c.mbf = S.MBF
            self.poses.append((h, np.ascontiguousarray(t.R.ravel()), t.t.copy(), t.Ow.copy()))
        self.best = np.zeros((K, m), np.int32); self.idx = np.zeros((K, m), np.int32); self.proj = np.zeros((K, m), ORBmatcher.PROJ_DTYPE)
        self.q = np.zeros(m, ORBmatcher.WQ_DTYPE)
        self.args = [_p(a) for a in (P, N, mind, maxd, desc)]
        self.pact = _p(active) if active is not None else None
        self.psf, self.psg = _p(S.SF), _p(S.INV_SIGMA2)

    def one_call(self):
        a = self.args
        assert self.L.orbm_fuse_keyframes(self.arr, self.K, 0, a[0], a[1], a[2], a[3], a[4], self.m, self.pact, TH, float(S.LOGSF), self.psf,
                                          self.psg, 8, _p(self.best), _p(self.idx), _p(self.proj)) == 0

    def singles(self):
        a, m = self.args, self.m
        for k, (h, Rk, tk, Ok) in enumerate(self.poses):
            assert self.L.orbm_project_points(1, a[0], a[1], a[2], a[3], m, _p(Rk), _p(tk), _p(Ok), _p(self.cam), S.MBF, 0.0, float(S.LOGSF),
                                              self.psf, 8, TH, _p(self.proj[k]), _p(self.q)) == 0
            assert self.L.orbm_frame_search_fuse(h, _p(self.q), a[4], m, self.psg, 8, _p(self.best[k]), _p(self.idx[k])) == 0

    def rows(self):
        return self.best.copy(), self.idx.copy(), self.proj.copy()

    def close(self):
        for h in self.frames:
            self.L.orbm_frame_destroy(h)
        self.frames = []


def time_forms(forms, batches, calls):
    for _ in range(3):
        for _, fn in forms:
            fn()
    times = {name: [] for name, _ in forms}
    for _ in range(batches):
        for name, fn in forms:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            times[name].append((time.perf_counter() - t0) / calls * 1e3)
    out = {}
    for name, ts in times.items():
        out[name + "_ms"] = round(float(np.median(ts)), 4)
        out[name + "_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
    return out


def whole_loop(K, batches):
    scene = S.random_scene(21, K=K, U=2000, nclutter=600, ndup=0, nnull=0)
    mt = ORBmatcher(0.8)
    dev = [t.device() for t in scene.targets]
    desc0 = scene.list_descriptors()

    def one():
        w = scene.world.clone()
        t0 = time.perf_counter()
        n = mt.fuse_keyframes(dev, scene.lst, scene.pos, scene.nrm, scene.mind, scene.maxd, desc0, S.LOGSF, S.SF, S.INV_SIGMA2, scene.th,
                              R.WorldOps(scene, w))
        return (time.perf_counter() - t0) * 1e3, n, w

    def sequential():
        w = scene.world.clone()
        ops = R.WorldOps(scene, w)
        li = np.maximum(scene.lst, 0)
        t0 = time.perf_counter()
        n = []
        for k, t in enumerate(scene.targets):
            ops.begin_target(k)
            proj, q = mt.project_points(1, scene.pos, scene.nrm, scene.mind, scene.maxd, t.R, t.t, t.Ow, S.cam_record(), t.mbf, S.LOGSF, S.SF, scene.th)
            best, idx = mt.frame_search_fuse(dev[k].frame, q, w.desc[li], S.INV_SIGMA2)
            n.append(mt.fuse_replay(scene.lst, proj["visible"], best, idx, ops))
        return (time.perf_counter() - t0) * 1e3, n, w
    (_, n1, w1), (_, n2, w2) = one(), sequential()
    assert n1 == n2 and w1.ops == w2.ops
    stats = dict(ORBmatcher._last_fuse_keyframes)
    t_one = [one()[0] for _ in range(batches)]; t_seq = [sequential()[0] for _ in range(batches)]
    active = sum(1 for h in scene.lst if not scene.world.bad[h])
    print(json.dumps({"loop_targets": K, "points": len(scene.lst), "keypoints": [len(t.desc) for t in scene.targets][:4], "nFused": n1,
                      "refreshes": stats["refreshes"], "waits": stats["waits"], "live_points": active,
                      "one_call_loop_ms": round(float(np.median(t_one)), 3), "one_call_loop_spread_ms": [round(min(t_one), 3), round(max(t_one), 3)],
                      "sequential_loop_ms": round(float(np.median(t_seq)), 3), "sequential_loop_spread_ms": [round(min(t_seq), 3), round(max(t_seq), 3)]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--targets", type=int, nargs="*", default=[1, 5, 10, 20, 40, 100])
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--masked", type=float, default=0.0, help="share of the pairs the mask leaves inactive (SearchInNeighbors: about 0.7)")
    ap.add_argument("--loop", type=int, default=0, help="time the whole loop over this many targets instead")
    a = ap.parse_args()
    if a.loop:
        return whole_loop(a.loop, a.batches)
    this = Build(SO_PATH)
    parent = Build(a.parent_lib) if a.parent_lib else None
    P, N, mind, maxd, desc, targets = timing_scene(max(a.targets), a.points, a.keypoints)
    for K in a.targets:
        rng = np.random.default_rng(K)
        active = (rng.random((K, a.points)) >= a.masked).astype(np.uint8) if a.masked > 0 else None
        this.prepare(P, N, mind, maxd, desc, targets[:K], active)
        forms = [("one_call", this.one_call), ("singles", this.singles)]
        if parent:
            parent.prepare(P, N, mind, maxd, desc, targets[:K], None)
            forms.append(("singles_parent", parent.singles))
        this.one_call(); got = this.rows()
        this.singles(); ref = this.rows()
        on = np.ones((K, a.points), bool) if active is None else active != 0
        assert all(np.array_equal(g[on], r[on]) for g, r in zip(got, ref))
        if parent:
            parent.singles()
            assert all(np.array_equal(g[on], r[on]) for g, r in zip(got, parent.rows()))
        line = {"targets": K, "points": a.points, "keypoints": a.keypoints, "masked": a.masked, "active_pairs": int(on.sum()),
                "visible": int((got[2]["visible"] > 0).sum()), "fused_candidates": int(((got[0] <= 45) & (got[1] >= 0)).sum()),
                "batches": a.batches, "calls_per_batch": a.calls}
        line.update(time_forms(forms, a.batches, a.calls))
        print(json.dumps(line), flush=True)
        this.close()
        if parent:
            parent.close()


if __name__ == "__main__":
    main()
