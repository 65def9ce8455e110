#!/usr/bin/env python3
"""Call time of orbm_essential_graph_env from Python, beside tools/essential_graph_time.py.
  default   against the dense entry orbm_essential_graph where both accept the graph: chain() of 40 / 128 / 256 / 438 keyframes, 20
            iterations, in one process; dense and envelope batches alternate, a figure is the median over the batches of the mean of
            the batch's calls with the spread (min .. max over batches) beside it.  `env_not_slower` holds when the envelope median is
            not above the dense median by more than the larger of the two spreads.
  --large   above the dense limit: tests/essential_graph_env_scenes.py long_chain() (chain() with planted loops among free keyframes)
            of 1,024 / 2,048 / 4,096 keyframes, 2 iterations: per call, per trial, launches per solve, live tiles, and the solver
            ALONE between device events (tools/llt_env_time.py's measurement on a diagonally dominant matrix with the scene's
            envelope; that tool holds the solver's own table over n and envelope, and against the dense solver).
No CPU figure: the dense restatement is no baseline at these sizes, and g2o's sparse solver does not run here.  One JSON line per size.

--profile: kernel times from a `rocprofv3 --kernel-trace --stats` pass of its own per size (a fresh child process runs the device
part under the profiler): every k_eg_* and k_llt_* kernel with its calls, mean and share, and per trial k_eg_assemble_env and the
solve."""
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
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

import essential_graph_env_scenes as env_scenes       # noqa: E402
import essential_graph_scenes as scenes               # noqa: E402
from llt_env_time import solver_ms                     # noqa: E402
from orb_slam2_e_amd import essential_graph as EG     # noqa: E402

SIZES, LARGE = [40, 128, 256, 438], [1024, 2048, 4096]


def batch(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def profile(sizes, large):
    for nact in sizes:
        with tempfile.TemporaryDirectory() as d:
            out = subprocess.check_output(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "eg", "--output-format", "csv", "--",
                                           sys.executable, os.path.abspath(__file__), "--batches", "1", "--calls", "2", "--size", str(nact), "--env-only"]
                                          + (["--large"] if large else []), stderr=subprocess.DEVNULL).decode()
            run = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            by = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    k = re.search(r"k_eg_\w+|k_llt_\w+|k_stage_copy", row.get("Name", ""))
                    if k:
                        e = by.setdefault(k.group(0), [0, 0.0]); e[0] += int(row["Calls"]); e[1] += float(row["TotalDurationNs"])
            total = sum(t for _, t in by.values()) or 1.0
            trials = run["trials"] * (2 + 2)                                        # the timed calls and the child's warm-up
            solve = sum(t for k, (c, t) in by.items() if k.startswith("k_llt_"))
            print(json.dumps({"nact": nact, "trials": run["trials"],
                              "per_trial_us": {"k_eg_assemble_env": round(by.get("k_eg_assemble_env", [0, 0.0])[1] / 1e3 / max(trials, 1), 2),
                                               "solve": round(solve / 1e3 / max(trials, 1), 2)},
                              "kernels": {k: {"calls": c, "mean_us": round(t / 1e3 / c, 2), "share": round(t / total, 4)}
                                          for k, (c, t) in sorted(by.items(), key=lambda r: -r[1][1])}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--size", type=int, default=None, help="one size instead of the list")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--env-only", action="store_true", help="no dense batches (the profiler's child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    todo = [a.size] if a.size else (LARGE if a.large else SIZES)
    if a.profile:
        return profile(todo, a.large)
    for nact in todo:
        g = env_scenes.long_chain(nact) if a.large else scenes.chain(nact)
        iters = 2 if a.large else 20
        p = EG.plan_env(g)
        got = EG.optimize_env(g, iters, want_stats=True)
        EG.optimize_env(g, iters)
        dense = not a.large and not a.env_only
        if dense:
            for _ in range(2):
                EG.optimize(g, iters)
        td, te = [], []
        for _ in range(a.batches):                                                  # alternating batches
            if dense:
                td.append(batch(lambda: EG.optimize(g, iters), a.calls))
            te.append(batch(lambda: EG.optimize_env(g, iters), a.calls))
        line = {"nact": nact, "n": 7 * nact, "nedges": int(len(g["e_v0"])), "iterations": got["iterations"], "trials": got["trials"], "waits": got["waits"],
                "row_tiles": p["row_tiles"], "live_tiles": p["live_tiles"], "launches_per_solve": p["launches"],
                "env_call_ms": round(float(np.median(te)), 3), "env_spread_ms": [round(min(te), 3), round(max(te), 3)],
                "env_ms_per_trial": round(float(np.median(te)) / max(got["trials"], 1), 3), "batches": a.batches, "calls_per_batch": a.calls}
        if dense:
            spread = max(max(td) - min(td), max(te) - min(te))
            line.update(dense_call_ms=round(float(np.median(td)), 3), dense_spread_ms=[round(min(td), 3), round(max(td), 3)],
                        dense_ms_per_trial=round(float(np.median(td)) / max(got["trials"], 1), 3),
                        env_not_slower=bool(np.median(te) <= np.median(td) + spread))
        if a.large and not a.env_only:
            line["solver_alone_ms"] = round(solver_ms(7 * nact, p["first"], reps=5, warmup=1)["env_ms"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
