#!/usr/bin/env python3
"""Call time of orbm_optimize_sim3 (Optimizer::OptimizeSim3 in one launch) from Python: 1 and 8 problems at n = 50 and n = 300
correspondences (1 px of noise, 10 % outliers, the start 5 degrees / 5 % off).  A figure is the median over batches of the mean of
10 calls, with the spread (min .. max over batches) beside it.  Beside it the CPU baseline by the project's convention: the
restatement (tests/sim3_opt_oracle.c) built -O3 -march=native -ffp-contract=off on one pinned thread of the same host, the problems
one after the other.  Prints one JSON line per shape.

--profile: kernel times from `rocprofv3 --kernel-trace --stats` passes of their own, one per shape (a fresh child process runs the
device part with 3 batches under the profiler; times under the profiler are longer than the call times above)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_opt_oracle as so                 # noqa: E402
import sim3_opt_scenes as scenes             # noqa: E402
from orb_slam2_e_amd import Sim3OptProblem, optimize_sim3   # noqa: E402
from orb_slam2_e_amd.sim3 import last_sim3_opt_waits        # noqa: E402

CPU_FLAGS = ("-O3", "-march=native")


def batches(fn, nb, calls):
    out = []
    for _ in range(nb):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shape", default=None, help="n,P: one shape instead of the four")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    shapes = [(n, P) for n in (50, 300) for P in (1, 8)] if a.shape is None else [tuple(int(v) for v in a.shape.split(","))]
    if a.profile:
        for n, P in shapes:                                     # one pass per shape: the statistics of a pass are per kernel name
            with tempfile.TemporaryDirectory() as d:
                subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sim3opt", "--output-format", "csv", "--",
                                       sys.executable, os.path.abspath(__file__), "--batches", "3", "--no-cpu", "--shape", f"{n},{P}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        m = re.search(r"k_sim3_optimize<\d+>", row.get("Name", ""))
                        if m:
                            print(json.dumps({"kernel": m.group(0), "n": n, "problems": P, "calls": int(row["Calls"]),
                                              "mean_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                              "max_us": round(float(row["MaxNs"]) / 1e3, 2)}), flush=True)
        return
    if not a.no_cpu:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})            # one pinned thread for the baseline (and the caller)
    for n, P in shapes:
        probs = [scenes.problem(900 + k, n) for k in range(P)]
        dev = [Sim3OptProblem(p["X1w"], p["X2w"], p["obs1"], p["obs2"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"],
                              p["R12"], p["t12"], p["s12"], p["th2"], p["fix_scale"]) for p in probs]
        got = optimize_sim3(dev, scenes.INV_SIGMA2)
        for _ in range(5):
            optimize_sim3(dev, scenes.INV_SIGMA2)
        td = batches(lambda: optimize_sim3(dev, scenes.INV_SIGMA2), a.batches, a.calls)
        line = {"problems": P, "n": n, "nin": [int(r.nin) for r, _ in got],
                "iterations": [list(r.iterations) for r, _ in got], "trials": [list(r.trials) for r, _ in got],
                "device_call_ms": round(float(np.median(td)), 4), "device_spread_ms": [round(min(td), 4), round(max(td), 4)],
                "waits": last_sim3_opt_waits(), "batches": a.batches, "calls_per_batch": a.calls}
        if not a.no_cpu:
            ref = [so.optimize(p, scenes.INV_SIGMA2, flags=CPU_FLAGS) for p in probs]
            assert all(abs(o["res"].nin - r.nin) <= 2 for o, (r, _) in zip(ref, got))
            tc = batches(lambda: [so.optimize(p, scenes.INV_SIGMA2, flags=CPU_FLAGS) for p in probs], a.batches, a.calls)
            line.update({"cpu_restatement_ms": round(float(np.median(tc)), 4), "cpu_spread_ms": [round(min(tc), 4), round(max(tc), 4)]})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
