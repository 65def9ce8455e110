#!/usr/bin/env python3
"""Call time of orbm_essential_graph (Optimizer::OptimizeEssentialGraph, 20 iterations) from Python at 40 / 128 / 256 / 438 keyframes
in the system with about 10 edges per keyframe (tests/essential_graph_scenes.py chain()).  Device and CPU batches alternate; a figure
is the median over the batches of the mean of the batch's calls, with the spread (min .. max over batches) beside it.  The CPU
baseline, by the project's convention, is the restatement (tests/essential_graph_oracle.c) built -O3 -march=native
-ffp-contract=off on one pinned thread of the same host; its dense LLT grows with the cube of the size, so the larger sizes run
fewer of its calls.  Prints one JSON line per size.

--profile: kernel times from `rocprofv3 --kernel-trace --stats` passes of their own, one per size (a fresh child process runs the
device part under the profiler; times under the profiler are longer than the call times above).  The line of a size then lists
every k_eg_* and k_llt_* kernel with its calls, mean and share, and per trial the time of k_eg_linearize (per iteration),
k_eg_assemble and the solve (the k_llt_* launches of one trial together)."""
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

import essential_graph_oracle as oracle       # noqa: E402
import essential_graph_scenes as scenes       # noqa: E402
from orb_slam2_e_amd import essential_graph as EG     # noqa: E402

CPU_FLAGS = ("-O3", "-march=native")
SIZES = [40, 128, 256, 438]
ITERATIONS = 20


def batch(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--size", type=int, default=None, help="one size instead of the four")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    todo = [a.size] if a.size else SIZES
    if a.profile:
        for nact in todo:
            with tempfile.TemporaryDirectory() as d:
                out = subprocess.check_output(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "eg", "--output-format", "csv", "--",
                                               sys.executable, os.path.abspath(__file__), "--batches", "1", "--calls", "2", "--no-cpu", "--size", str(nact)],
                                              stderr=subprocess.DEVNULL).decode()
                run = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
                rows = []
                for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        k = re.search(r"k_eg_\w+|k_llt_\w+|k_stage_copy", row.get("Name", ""))
                        if k:
                            rows.append((k.group(0), int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["TotalDurationNs"])))
                total = sum(r[3] for r in rows) or 1.0
                by = {}
                for k, c, us, t in rows:
                    e = by.setdefault(k, [0, 0.0]); e[0] += c; e[1] += t
                ncalls = 2 + 4                                                          # the timed calls and the warm-up of the child
                trials, iters = run["trials"] * ncalls, run["iterations"] * ncalls
                llt = sum(t for k, (c, t) in by.items() if k.startswith("k_llt_"))
                print(json.dumps({"nact": nact, "nedges": run["nedges"], "trials": run["trials"], "iterations": run["iterations"],
                                  "per_iteration_us": {"k_eg_linearize": round(by.get("k_eg_linearize", [0, 0.0])[1] / 1e3 / max(iters, 1), 2)},
                                  "per_trial_us": {"k_eg_assemble": round(by.get("k_eg_assemble", [0, 0.0])[1] / 1e3 / max(trials, 1), 2),
                                                   "solve": round(llt / 1e3 / max(trials, 1), 2)},
                                  "kernels": {k: {"calls": c, "mean_us": round(t / 1e3 / c, 2), "share": round(t / total, 4)}
                                              for k, (c, t) in sorted(by.items(), key=lambda r: -r[1][1])}}), flush=True)
        return
    if not a.no_cpu:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})            # one pinned thread for the baseline (and the caller)
    for nact in todo:
        g = scenes.chain(nact)
        got = EG.optimize(g, ITERATIONS, want_stats=True)
        for _ in range(3):
            EG.optimize(g, ITERATIONS)
        cpu_calls = 0 if a.no_cpu else (2 if nact <= 128 else 1)
        cpu_batches = 0 if a.no_cpu else (max(a.batches // 2, 2) if nact <= 256 else 1)
        td, tc = [], []
        ref = None
        for b in range(a.batches):                                                  # alternating batches
            td.append(batch(lambda: EG.optimize(g, ITERATIONS), a.calls))
            if b < cpu_batches:
                if ref is None:
                    ref = oracle.run(g, ITERATIONS, flags=CPU_FLAGS, want_system=False)
                tc.append(batch(lambda: oracle.run(g, ITERATIONS, flags=CPU_FLAGS, want_system=False), cpu_calls))
        line = {"nact": nact, "n": 7 * nact, "nedges": int(len(g["e_v0"])), "iterations": got["iterations"], "trials": got["trials"], "waits": got["waits"],
                "device_call_ms": round(float(np.median(td)), 3), "device_spread_ms": [round(min(td), 3), round(max(td), 3)],
                "device_ms_per_trial": round(float(np.median(td)) / max(got["trials"], 1), 3), "batches": a.batches, "calls_per_batch": a.calls}
        if tc:
            line.update(cpu_restatement_ms=round(float(np.median(tc)), 3), cpu_spread_ms=[round(min(tc), 3), round(max(tc), 3)], cpu_batches=len(tc),
                        cpu_calls_per_batch=cpu_calls, cpu_trials=ref["trials"], cpu_ms_per_trial=round(float(np.median(tc)) / max(ref["trials"], 1), 3),
                        same_integers=bool(ref["iterations"] == got["iterations"] and ref["trials"] == got["trials"]),
                        device_faster=bool(np.median(td) < np.median(tc)))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
