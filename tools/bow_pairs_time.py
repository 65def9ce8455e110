#!/usr/bin/env python3
"""Call time of SearchByBoW against K candidate keyframes (the first stage of Tracking::Relocalization) on resident frames:
  (a) one call of orbm_frame_search_by_bow_pairs over the K pairs;
  (b) K x orbm_frame_search_by_bow from this build;
  (c) with --parent-lib PATH (a build of the parent commit's library): K x orbm_frame_search_by_bow from that build, in the same
      process and the same alternation: this change touches the kernels (b) runs.
The README's shape: synth_bow_case 2000 x 2100 features, 90 nodes; ONE current frame is the second frame of every pair, the K
keyframes are its first set under per-keyframe valid and stop-word masks (tests/bow_pairs_scenes.shared_second).  K = 1, 5, 10, 20.
All three go through bare ctypes with preallocated rows, so they differ in the library calls alone.  --ratio sets mfNNratio (0.6:
the README row's matcher), --noise puts the keyframes under 1 % bit noise, which makes long dependency chains among the case's
look-alikes (the resolver then iterates tens of times: the expensive end).
The forms alternate in one process; a figure is the median over batches of the mean of 10 calls, with the spread (min .. max over
batches) beside it.  Prints one JSON line per K.

Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python tools/bow_pairs_time.py --batches 3` in a run of its own and
read k_list_fill_pairs + k_resolve_par_pairs against k_list_fill + k_resolve_par from the statistics."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import bow_pairs_scenes as B                                       # noqa: E402
from orb_slam2_e_amd._lib import SO_PATH, lib, prototypes, ptr as _p   # noqa: E402
from orb_slam2_e_amd.matcher import _CBowPair                      # noqa: E402

BOUNDS = (0.0, 0.0, 640.0, 480.0)


class Build:
    """One build of the library through bare ctypes, outputs preallocated: the three forms then differ in the library calls alone
    (the Python wrappers' array conversions cost as much as a search)."""

    def __init__(self, path, ratio):
        self.L = lib() if path == SO_PATH else C.CDLL(path)
        self.ratio = ratio
        for name in ("orbm_frame_create", "orbm_frame_search_by_bow", "orbm_frame_destroy", "orbm_frame_search_by_bow_pairs"):
            if hasattr(self.L, name):
                fn = getattr(self.L, name)
                fn.restype, fn.argtypes = prototypes()[name]
        self.frames = {}

    def frame(self, side):
        if id(side) not in self.frames:
            h = C.c_void_p()
            assert self.L.orbm_frame_create(_p(side.kps), _p(side.desc), side.n, None, *BOUNDS, C.byref(h)) == 0
            self.frames[id(side)] = (side, h)
        return self.frames[id(side)][1]

    def prepare(self, pairs):
        """the pairs as the C struct array, with their output rows"""
        self.rows = [(np.zeros(p.s1.n, np.int32), np.zeros(p.s2.n, np.int32)) for p in pairs]
        self.nm = np.zeros(len(pairs), np.int32)
        self.arr = (_CBowPair * len(pairs))()
        for c, p, (m12, m21) in zip(self.arr, pairs, self.rows):
            a, b = p.s1, p.s2
            c.frame1, c.nodes1, c.off1, c.items1, c.nn1, c.valid1 = self.frame(a).value, _p(a.fv[0]).value, _p(a.fv[1]).value, _p(a.fv[2]).value, len(a.fv[0]), _p(a.valid).value
            c.frame2, c.nodes2, c.off2, c.items2, c.nn2, c.valid2 = self.frame(b).value, _p(b.fv[0]).value, _p(b.fv[1]).value, _p(b.fv[2]).value, len(b.fv[0]), None
            c.match12, c.match21 = _p(m12).value, _p(m21).value
        self.pnm = _p(self.nm)

    def one_call(self):
        assert self.L.orbm_frame_search_by_bow_pairs(self.arr, len(self.rows), 45, 0, self.ratio, 1, self.pnm) == 0
        return self.nm.tolist()

    def singles(self):
        out = []
        nm = C.c_int(0)
        for c in self.arr:
            assert self.L.orbm_frame_search_by_bow(c.frame1, c.nodes1, c.off1, c.items1, c.nn1, c.valid1, c.frame2, c.nodes2, c.off2, c.items2, c.nn2,
                                                   None, 45, 0, self.ratio, 1, c.match12, c.match21, C.byref(nm)) == 0
            out.append(nm.value)
        return out

    def close(self):
        for _, h in self.frames.values():
            self.L.orbm_frame_destroy(h)
        self.frames = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 5, 10, 20])
    ap.add_argument("--ratio", type=float, default=0.6, help="mfNNratio (0.6: the README row's matcher; the reference relocalises with 0.75)")
    ap.add_argument("--parent-first", action="store_true", help="time the parent build's form first in every round (an order effect would show)")
    ap.add_argument("--noise", action="store_true", help="keyframes under 1 %% bit noise: long dependency chains among the look-alikes")
    a = ap.parse_args()
    this = Build(SO_PATH, a.ratio)
    parent = Build(a.parent_lib, a.ratio) if a.parent_lib else None
    allpairs = B.shared_second(list(range(max(a.pairs))), 2000, 2100, 90, noise=a.noise)
    for K in a.pairs:
        pairs = allpairs[:K]
        this.prepare(pairs)
        forms = [("one_call", this.one_call), ("singles", this.singles)]
        if parent:
            parent.prepare(pairs)
            forms.append(("singles_parent", parent.singles))
            if a.parent_first:
                forms.reverse()
        got = this.one_call()
        waits = this.L.orbm_debug_last_bow_pairs_waits()
        rows = [(m12.copy(), m21.copy()) for m12, m21 in this.rows]
        assert got == this.singles() and all(np.array_equal(r[0], s[0]) and np.array_equal(r[1], s[1]) for r, s in zip(rows, this.rows))
        assert not parent or (got == parent.singles() and all(np.array_equal(r[0], s[0]) for r, s in zip(rows, parent.rows)))
        for _ in range(3):
            for _, fn in forms:
                fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.batches):
            for name, fn in forms:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                times[name].append((time.perf_counter() - t0) / a.calls * 1e3)
        line = {"features": [2000, 2100], "nodes": 90, "ratio": a.ratio, "noise": a.noise, "pairs": K, "nmatches": got, "waits_one_call": waits,
                "batches": a.batches, "calls_per_batch": a.calls}
        for name, ts in times.items():
            line[name + "_ms"] = round(float(np.median(ts)), 4)
            line[name + "_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
        print(json.dumps(line), flush=True)
    this.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
