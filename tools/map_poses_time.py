#!/usr/bin/env python3
"""Call time of the whole-map relocalisation search under P poses (PnPsolver::iterate's second stage) on a resident frame:
  (a) one call of orbm_frame_search_by_projection_map_poses on a map snapshot;
  (b) P x orbm_frame_search_by_projection_map, the map arrays passed with every call.
With --parent-lib PATH (a build of the parent commit's library) form (b) is also timed on that build, in the same process and the
same alternation: this change touches the kernels (b) runs.  n = 2000 keypoints; m = 5000 and 20000 map points; P = 1, 5, 10.
The forms alternate in one process; a figure is the median over batches of the mean of 10 calls, with the spread (min .. max over
batches) beside it.  Prints one JSON line per (m, P).

Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python tools/map_poses_time.py --batches 3` in a run of its own and
read k_map_search_poses against k_map_frustum + k_win_best + k_reloc_accept from the statistics."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_poses_scenes as scenes                                  # noqa: E402
from orb_slam2_e_amd import Frame, MapSnapshot, ORBmatcher         # noqa: E402
from orb_slam2_e_amd._lib import prototypes, ptr as _p             # noqa: E402


class ParentBuild:
    """orbm_frame_create / orbm_frame_search_by_projection_map / orbm_frame_destroy of another build of the library"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        for name in ("orbm_frame_create", "orbm_frame_search_by_projection_map", "orbm_frame_destroy"):
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = prototypes()[name]

    def frame(self, kps, desc):
        h = C.c_void_p()
        assert self.L.orbm_frame_create(_p(kps), _p(desc), len(kps), None, 0.0, 0.0, 640.0, 480.0, C.byref(h)) == 0
        return h

    def search(self, h, s, p, matched, proj):
        nm = C.c_int(0)
        R = np.ascontiguousarray(s["Rcw"][p], np.float64); t = np.ascontiguousarray(s["tcw"][p], np.float64)
        rc = self.L.orbm_frame_search_by_projection_map(h, _p(s["has_mp"]), _p(s["pos"]), _p(s["nrm"]), _p(s["mind"]), _p(s["maxd"]), _p(s["mp_desc"]),
                                                        len(s["pos"]), _p(R), _p(t), _p(s["cam"]), _p(s["sf"]), len(s["sf"]), s["th"], 0.6, 60,
                                                        _p(matched), C.byref(nm), _p(proj))
        assert rc == 0
        return nm.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    M = ORBmatcher(0.6)
    parent = ParentBuild(a.parent_lib) if a.parent_lib else None
    for m in (5000, 20000):
        for P in (1, 5, 10):
            s = scenes.scene(5, m, 2000, P, 15.0)
            F = Frame(s["kps"], s["desc"], (0.0, 0.0, 640.0, 480.0))
            snap = MapSnapshot(s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"])
            hp = parent.frame(s["kps"], s["desc"]) if parent else None
            mk = np.zeros(2000, np.int32); pj = np.zeros((m, 4), np.float32)

            def one_call():
                return M.frame_search_by_projection_map_poses(F, s["has_mp"], snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"], want_proj=False)

            def chained():
                return [M.frame_search_by_projection_map(F, s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], s["Rcw"][p],
                                                         s["tcw"][p], s["cam"], s["sf"], s["th"])[1] for p in range(P)]

            def chained_parent():
                return [parent.search(hp, s, p, mk, pj) for p in range(P)]

            forms = [("one_call", one_call), ("chained", chained)] + ([("chained_parent", chained_parent)] if parent else [])
            got = one_call()
            assert got[1].tolist() == chained() and (not parent or got[1].tolist() == chained_parent())
            for _ in range(3):
                for _, fn in forms:
                    fn()
            one_call(); waits = ORBmatcher.last_map_poses_waits()
            times = {name: [] for name, _ in forms}
            for _ in range(a.batches):
                for name, fn in forms:
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    times[name].append((time.perf_counter() - t0) / a.calls * 1e3)
            line = {"map_points": m, "keypoints": 2000, "poses": P, "nmatches": got[1].tolist(), "waits_one_call": waits, "batches": a.batches,
                    "calls_per_batch": a.calls}
            for name, ts in times.items():
                line[name + "_ms"] = round(float(np.median(ts)), 4)
                line[name + "_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
            print(json.dumps(line), flush=True)
            F.close(); snap.close()
            if parent:
                parent.L.orbm_frame_destroy(hp)


if __name__ == "__main__":
    main()
