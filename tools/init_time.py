#!/usr/bin/env python3
"""Call time of orbm_init_find_models (FindHomography + FindFundamental, 200 hypotheses each, in one launch) and of
orbm_init_reconstruct_f (ReconstructF: four CheckRT passes in one launch) from Python, at n = 100, 300 and 1000 matches.  A figure
is the median over batches of the mean of 10 calls, with the spread (min .. max over batches) beside it.  Beside it the CPU
baseline by the project's convention: the restatement (tests/init_oracle.c) built -O3 -march=native -ffp-contract=off on one pinned
thread of the same host -- and, for the H / F pair, on two threads as the reference runs it (src/Initializer.cc:99-109).  Prints one
JSON line per shape.

--profile: kernel times from one `rocprofv3 --kernel-trace --stats` pass of its own (a fresh child process runs the device part
with 3 batches under the profiler; times under the profiler are longer than the call times above)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import init_oracle as io                     # noqa: E402
import init_scenes as scenes                 # noqa: E402
from orb_slam2_e_amd import find_models, last_init_waits, reconstruct_f    # noqa: E402

CPU_FLAGS = ("-O3", "-march=native")


def batches(fn, nb, calls):
    out = []
    for _ in range(nb):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return out


def fig(t):
    return round(float(np.median(t)), 4), [round(min(t), 4), round(max(t), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        with tempfile.TemporaryDirectory() as d:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "init", "--output-format", "csv", "--",
                                   sys.executable, os.path.abspath(__file__), "--batches", "3", "--no-cpu"], stdout=subprocess.DEVNULL)
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    name = re.search(r"k_init_\w+", row.get("Name", ""))          # (the names carry their anonymous namespace in front)
                    if name:
                        print(json.dumps({"kernel": name.group(0), "calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                          "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}), flush=True)
        return
    cpus = sorted(os.sched_getaffinity(0))
    for n in (100, 300, 1000):
        s = scenes.scene(600 + n, n, 200, "general", noise=0.5, outliers=0.2, extra=n // 2)
        args = (s["keys1"], s["keys2"], s["matches"], s["sets"])
        got = find_models(*args)
        for _ in range(5):
            find_models(*args)
        td, sd = fig(batches(lambda: find_models(*args), a.batches, a.calls))
        rec = (s["keys1"], s["keys2"], s["matches"], got["inliersF"], got["F21"], s["K"])
        reconstruct_f(*rec)
        tr, sr = fig(batches(lambda: reconstruct_f(*rec), a.batches, a.calls))
        line = {"n": n, "hypotheses": 200, "SH": float(got["SH"]), "SF": float(got["SF"]), "inliersF": int(got["inliersF"].sum()),
                "find_models_ms": td, "find_models_spread_ms": sd, "reconstruct_f_ms": tr, "reconstruct_f_spread_ms": sr, "waits": last_init_waits(),
                "batches": a.batches, "calls_per_batch": a.calls}
        if not a.no_cpu:
            one = lambda model: io.find_model(model, *args, flags=CPU_FLAGS)
            ref = [one(0), one(1)]
            assert abs(float(ref[1]["S"]) - float(got["SF"])) <= 1e-3 * abs(float(ref[1]["S"])) + 1e-3

            def two_threads():                       # ctypes releases the interpreter lock inside the call
                th = [threading.Thread(target=one, args=(m,)) for m in (0, 1)]
                for t in th:
                    t.start()
                for t in th:
                    t.join()

            os.sched_setaffinity(0, set(cpus[:2]))
            t2, s2 = fig(batches(two_threads, a.batches, a.calls))
            os.sched_setaffinity(0, {cpus[0]})        # one pinned thread
            t1, s1 = fig(batches(lambda: (one(0), one(1)), a.batches, a.calls))
            tc, sc = fig(batches(lambda: io.reconstruct_f(*rec, flags=CPU_FLAGS), a.batches, a.calls))
            os.sched_setaffinity(0, set(cpus))
            line.update({"cpu_find_models_one_thread_ms": t1, "cpu_find_models_one_thread_spread_ms": s1, "cpu_find_models_two_threads_ms": t2,
                         "cpu_find_models_two_threads_spread_ms": s2, "cpu_reconstruct_f_ms": tc, "cpu_reconstruct_f_spread_ms": sc})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
