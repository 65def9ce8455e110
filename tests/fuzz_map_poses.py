#!/usr/bin/env python3
"""Seed sweep of tests/test_gpu_map_poses.py::test_every_row_equals_the_oracle (not collected by pytest; needs a GPU):
python tests/fuzz_map_poses.py [seeds]  -- random (m, n, P, th) per seed, every row against the oracle called once per pose."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from map_poses_scenes import oracle_rows, scene                     # noqa: E402
from orb_slam2_e_amd import Frame, MapSnapshot, ORBmatcher          # noqa: E402


def main():
    nseeds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    M = ORBmatcher(0.6)
    for seed in range(100, 100 + nseeds):
        rng = np.random.default_rng(seed)
        sc = (seed, int(rng.integers(17, 3000)), int(rng.integers(20, 1500)), int(rng.integers(1, 17)), float(rng.choice([1.0, 3.0, 15.0])))
        s = scene(*sc)
        F = Frame(s["kps"], s["desc"], (0.0, 0.0, 640.0, 480.0)); snap = MapSnapshot(s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"])
        got = M.frame_search_by_projection_map_poses(F, s["has_mp"], snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"])
        ref = oracle_rows(*sc)
        ok = np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
        print(sc, "nmatches", got[1].tolist(), "ok" if ok else "MISMATCH", flush=True)
        F.close(); snap.close()
        if not ok:
            return 1
    print("fuzz_map_poses ok:", nseeds, "seeds")
    return 0


if __name__ == "__main__":
    sys.exit(main())
