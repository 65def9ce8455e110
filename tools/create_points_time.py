#!/usr/bin/env python3
"""Call time of LocalMapping::CreateNewMapPoints' neighbour loop on resident keyframes:
  (a) one call of orbm_create_new_map_points;
  (b) the chained form: K x orbm_frame_search_for_triangulation, each followed on the host by the CPU restatement's triangulation
      of its matches (tests/create_points_oracle.c) and the update of the "owns a point" mask.
2000-keypoint stereo and monocular scenes, K = 10 and 20.  The two forms alternate in one process; a figure is the median over
batches of the mean of 10 calls, with the spread (min .. max over batches) beside it.  Prints one JSON line per scene.

Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python tools/create_points_time.py --batches 3` in a run of its
own and read k_create_points / k_triang_frames from the statistics."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import create_points_oracle as cpo            # noqa: E402
import create_points_scenes as scenes         # noqa: E402
from orb_slam2_e_amd import Frame, ORBmatcher, TriangKeyFrame   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = ORBmatcher(0.6, False)
    for mono in (False, True):
        for K in (10, 20):
            s = scenes.random_scene(400 + K + mono, 2000, K, mono=mono)
            cur = s["cur"]
            frames = [Frame(kf["kps"], kf["desc"], (0.0, 0.0, 640.0, 480.0), kf["uright"]) for kf in [cur] + s["neigh"]]
            tcur = TriangKeyFrame(frames[0], cur["Tcw"], cur["cam"], cur["fv"], cur["has"], cur["depth"])
            tnb = [TriangKeyFrame(f, nb["Tcw"], nb["cam"], nb["fv"], nb["has"], nb["depth"], nb["F12"], nb["ex"], nb["ey"])
                   for f, nb in zip(frames[1:], s["neigh"])]
            ST = cpo.STATUS

            def one_call():
                return ORBmatcher.CreateNewMapPoints(tcur, tnb, s["sf"], s["sg"], s["scale_factor"])

            def chained():
                has = cur["has"].copy(); nnew = 0
                for k, nb in enumerate(s["neigh"]):
                    _, _, m12 = m.frame_search_for_triangulation(frames[0], cur["fv"], has, frames[1 + k], nb["fv"], nb["has"], nb["F12"], nb["ex"],
                                                                 nb["ey"], s["sf"], s["sg"], False)
                    i1 = np.nonzero(m12 >= 0)[0]
                    r = cpo.triangulate_pairs(s, k, i1, m12[i1])
                    made = i1[r["status"] == ST["CREATED"]]
                    has[made] = True; nnew += len(made)
                return nnew

            got = one_call()
            assert chained() == got.nnew or abs(chained() - got.nnew) <= 0.02 * got.nnew
            for _ in range(3):
                one_call(); chained()
            ta, tb = [], []
            for _ in range(a.batches):
                for fn, out in ((one_call, ta), (chained, tb)):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    out.append((time.perf_counter() - t0) / a.calls * 1e3)
            print(json.dumps({"scene": "mono" if mono else "stereo", "K": K, "keypoints": 2000, "nnew": got.nnew,
                              "one_call_ms": round(float(np.median(ta)), 4), "one_call_spread_ms": [round(min(ta), 4), round(max(ta), 4)],
                              "chained_ms": round(float(np.median(tb)), 4), "chained_spread_ms": [round(min(tb), 4), round(max(tb), 4)],
                              "waits_one_call": ORBmatcher.last_create_points_waits(), "batches": a.batches, "calls_per_batch": a.calls}), flush=True)
            for f in frames:
                f.close()


if __name__ == "__main__":
    main()
