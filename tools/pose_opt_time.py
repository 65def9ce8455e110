"""Latency of the device PoseOptimization (orbm_pose.hip): one 500-edge call from Python (host arrays and resident frame), a
64 x 500-edge batch in one launch, and the CPU restatement (tests/pose_only_oracle.c, one host thread) as the CPU column.
Per-kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/pose_opt_time.py`.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pose_only_oracle as po  # noqa: E402
import pose_only_scene as ps  # noqa: E402
from orb_slam2_e_amd import pose_optimization, pose_optimization_batch  # noqa: E402
from orb_slam2_e_amd.extractor import KP_DTYPE  # noqa: E402
from orb_slam2_e_amd.matcher import Frame  # noqa: E402


def _median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=500)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    p = ps.make_problem(3, a.edges, stereo_frac=0.4, outlier_frac=0.2, fill=1.0)
    call = lambda fr=None: pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"],
                                             p["Tcw"], frame=fr)
    res = call()
    for _ in range(5):
        call()
    single = _median_ms(call, a.reps)
    k = np.zeros(a.edges, KP_DTYPE)
    k["x"], k["y"], k["octave"] = p["kp_xy"][:, 0], p["kp_xy"][:, 1], p["octave"]
    fr = Frame(k, np.zeros((a.edges, 32), np.uint8), (-1e4, -1e4, 1e4, 1e4), p["uright"])
    resident = _median_ms(lambda: call(fr), a.reps)
    fr.close()
    probs = [ps.make_problem(100 + b, a.edges, stereo_frac=0.4, outlier_frac=0.2, fill=1.0) for b in range(a.batch)]
    pose_optimization_batch(probs, ps.CAM, ps.inv_level_sigma2())
    batch = _median_ms(lambda: pose_optimization_batch(probs, ps.CAM, ps.inv_level_sigma2()), max(5, a.reps // 5))
    cpu = _median_ms(lambda: po.run(p), max(5, a.reps // 5))
    st = res[3]
    print(json.dumps({"edges": a.edges, "single_call_ms": round(single, 4), "resident_call_ms": round(resident, 4),
                      f"batch{a.batch}_ms": round(batch, 4), "cpu_restatement_ms": round(cpu, 4),
                      "iterations": list(st.iterations), "trials": list(st.trials)}))


if __name__ == "__main__":
    main()
