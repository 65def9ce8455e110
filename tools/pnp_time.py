#!/usr/bin/env python3
"""Call time of orbm_pnp_hypotheses (every EPnP RANSAC hypothesis of PnPsolver in one call) from Python: 1 and 5 candidates, 300
hypotheses each, n = 50 and n = 300 correspondences.  A figure is the median over batches of the mean of 10 calls, with the
spread (min .. max over batches) beside it.  Beside it the CPU baseline by the project's convention: the restatement
(tests/pnp_oracle.c) built -O3 -march=native -ffp-contract=off on one pinned thread of the same host, the candidates one after
the other.  Prints one JSON line per shape.

--profile: kernel times from one `rocprofv3 --kernel-trace --stats` pass of its own (a fresh child process runs the device part
with 3 batches under the profiler; times under the profiler are longer than the call times above)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import pnp_oracle as po                      # noqa: E402
import pnp_scenes as scenes                  # noqa: E402
from orb_slam2_e_amd import PnpProblem, pnp_hypotheses      # noqa: E402
from orb_slam2_e_amd.pnp import last_pnp_waits              # noqa: E402

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
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        with tempfile.TemporaryDirectory() as d:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "pnp", "--output-format", "csv", "--",
                                   sys.executable, os.path.abspath(__file__), "--batches", "3", "--no-cpu"], stdout=subprocess.DEVNULL)
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if "pnp" in row.get("Name", ""):
                        print(json.dumps({"kernel": next((w for w in row["Name"].replace("(", " ").replace(":", " ").split() if w.startswith("k_pnp")), row["Name"]), "calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                          "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}), flush=True)
        return
    if not a.no_cpu:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})            # one pinned thread for the baseline (and the caller)
    for n in (50, 300):
        for P in (1, 5):
            probs = [scenes.problem(700 + n + k, n, 300, outliers=0.4) for k in range(P)]
            dev = [PnpProblem(p["Xw"], p["uv"], p["octave"], p["cam"], p["sets"], p["min_inliers"], p["th2"]) for p in probs]
            got = pnp_hypotheses(dev, scenes.SIGMA2)
            for _ in range(5):
                pnp_hypotheses(dev, scenes.SIGMA2)
            td = batches(lambda: pnp_hypotheses(dev, scenes.SIGMA2), a.batches, a.calls)
            line = {"candidates": P, "hypotheses": 300, "n": n, "best_count": int(max(h["ninliers"].max() for h, _, _ in got)),
                    "records": int(sum(h["refined"].sum() for h, _, _ in got)),
                    "device_call_ms": round(float(np.median(td)), 4), "device_spread_ms": [round(min(td), 4), round(max(td), 4)],
                    "waits": last_pnp_waits(), "batches": a.batches, "calls_per_batch": a.calls}
            if not a.no_cpu:
                ref = [po.hypotheses(p, scenes.SIGMA2, flags=CPU_FLAGS) for p in probs]
                assert all(np.array_equal(r["ninliers"], h["ninliers"]) for r, (h, _, _) in zip(ref, got))
                tc = batches(lambda: [po.hypotheses(p, scenes.SIGMA2, flags=CPU_FLAGS) for p in probs], max(3, a.batches // 3), max(2, a.calls // 5))
                line.update({"cpu_restatement_ms": round(float(np.median(tc)), 4), "cpu_spread_ms": [round(min(tc), 4), round(max(tc), 4)]})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
