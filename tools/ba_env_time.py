#!/usr/bin/env python3
"""Call time of orbm_global_bundle_adjustment_env from Python; the method of tools/llt_time.py and
tools/essential_graph_env_time.py: alternating batches in one process, a figure is the median over the batches of the mean of the
batch's calls, with the spread (min .. max over batches) beside it.
  default   against the dense entry orbm_global_bundle_adjustment on graphs both accept: tests/ba_scenes.make with 64 / 128 / 256 / 512
            keyframes (5 points each, the shapes of tests/ba_large_scenes.py: every keyframe pair shares points, a FULL envelope, so
            the zeroing pass and the packed tiles are new work and nothing is saved), and tests/ba_env_scenes.make with 512 keyframes
            (a band).  `env_not_slower` holds when the envelope median is not above the dense median by more than the larger of the
            two spreads; `env_over_dense` is the ratio of the medians either way.
  --large   above the dense limit: banded maps of 1,024 / 2,048 / 4,096 keyframes with a planted loop, 3 iterations: per call, per
            trial, live tiles, launches per solve, and the solver ALONE between device events (tools/llt_env_time.py's measurement
            on a diagonally dominant matrix with the scene's envelope).
No CPU figure: g2o's sparse solver has never run here, so the CPU comparison is unmeasured; the dense restatement is no baseline at
these sizes.  The launch chain (about 43 us per launch, up to 4 nt - 1 launches per solve) is the known floor of a trial.  One JSON
line per size.

--profile: kernel times from a `rocprofv3 --kernel-trace --stats` pass of its own per size (a fresh child process runs the device
part under the profiler): every k_ba_* and k_llt_* kernel and the fill with its calls, mean and share; per trial the fill,
k_ba_schur_env and the solve; per round k_ba_activate."""
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

import ba_env_scenes                                   # noqa: E402
import ba_scenes                                       # noqa: E402
from llt_env_time import solver_ms                     # noqa: E402
from orb_slam2_e_amd import bundle                     # noqa: E402

SIZES, LARGE = ["full64", "full128", "full256", "full512", "band512"], ["band1024", "band2048", "band4096"]


def graph(name):
    kind, nk = name[:4], int(name[4:])
    if kind == "full":
        return ba_scenes.make(nfree=nk, nfixed=0, npoints=5 * nk, seed=900 + nk, obs_per_point=(3, 8), kf0_fixed=True)
    loops = (((2, 5), (nk - 16, nk - 12), 6),) if nk > 512 else ()
    return ba_env_scenes.make(nfree=nk, seed=900 + nk, w=8 if nk >= 4096 else 6, loops=loops)


def batch(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def profile(names):
    for name in names:
        with tempfile.TemporaryDirectory() as d:
            out = subprocess.check_output(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ba", "--output-format", "csv", "--",
                                           sys.executable, os.path.abspath(__file__), "--batches", "1", "--calls", "2", "--size", name, "--env-only"],
                                          stderr=subprocess.DEVNULL).decode()
            run = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            by = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    k = re.search(r"k_ba_\w+|k_llt_\w+|k_stage_copy|fill\w*", row.get("Name", ""), re.I)
                    if k:
                        e = by.setdefault(k.group(0), [0, 0.0]); e[0] += int(row["Calls"]); e[1] += float(row["TotalDurationNs"])
            total = sum(t for _, t in by.values()) or 1.0
            calls = 2 + 2                                                           # the timed calls and the child's warm-up
            trials = run["trials"] * calls
            solve = sum(t for k, (c, t) in by.items() if k.startswith("k_llt_"))
            fill = sum(t for k, (c, t) in by.items() if k.lower().startswith("fill"))
            print(json.dumps({"scene": name, "trials": run["trials"], "kernel_ms_per_call": round(total / 1e6 / calls, 3),
                              "per_trial_us": {"fill": round(fill / 1e3 / max(trials, 1), 2),
                                               "k_ba_schur_env": round(by.get("k_ba_schur_env", [0, 0.0])[1] / 1e3 / max(trials, 1), 2),
                                               "solve": round(solve / 1e3 / max(trials, 1), 2)},
                              "per_round_us": {"k_ba_activate": round(by.get("k_ba_activate", [0, 0.0])[1] / 1e3 / calls, 2)},
                              "solve_share": round(solve / total, 4), "k_ba_activate_share": round(by.get("k_ba_activate", [0, 0.0])[1] / total, 5),
                              "kernels": {k: {"calls": c, "mean_us": round(t / 1e3 / c, 2), "share": round(t / total, 4)}
                                          for k, (c, t) in sorted(by.items(), key=lambda r: -r[1][1])}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--size", default=None, help="one scene (full64 .. full512, band512 .. band4096) instead of the list")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--env-only", action="store_true", help="no dense batches, no solver-alone figure (the profiler's child)")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    todo = [a.size] if a.size else (LARGE if a.large else SIZES)
    if a.profile:
        return profile(todo)
    for name in todo:
        g = graph(name)
        large = g["nfree"] > 512
        opt = bundle.global_options(3 if large else 10, False)
        p = bundle.plan_global_env(g)
        got = bundle.run_global_env(g, opt, want_stats=True)
        bundle.run_global_env(g, opt)
        dense = not large and not a.env_only
        if dense:
            for _ in range(2):
                bundle.run_global(g, opt)
        td, te = [], []
        for _ in range(a.batches):                                                  # alternating batches
            if dense:
                td.append(batch(lambda: bundle.run_global(g, opt), a.calls))
            te.append(batch(lambda: bundle.run_global_env(g, opt), a.calls))
        trials = sum(got["trials"])
        n = 6 * int((p["pose_class"][:g["nfree"]] == 0).sum())
        line = {"scene": name, "nfree": g["nfree"], "n": n, "npoints": len(g["points"]), "nedges": len(g["e_point"]), "listed_blocks": len(p["blk_i1"]),
                "iterations": got["iterations"][0], "trials": trials, "waits": got["waits"], "row_tiles": len(p["first"]),
                "live_tiles": p["live_tiles"], "full_triangle_tiles": len(p["first"]) * (len(p["first"]) + 1) // 2, "launches_per_solve": p["launches"],
                "env_call_ms": round(float(np.median(te)), 3), "env_spread_ms": [round(min(te), 3), round(max(te), 3)],
                "env_ms_per_trial": round(float(np.median(te)) / max(trials, 1), 3), "batches": a.batches, "calls_per_batch": a.calls}
        if dense:
            spread = max(max(td) - min(td), max(te) - min(te))
            line.update(dense_call_ms=round(float(np.median(td)), 3), dense_spread_ms=[round(min(td), 3), round(max(td), 3)],
                        env_over_dense=round(float(np.median(te) / np.median(td)), 4), env_not_slower=bool(np.median(te) <= np.median(td) + spread))
        if large and not a.env_only:
            line["solver_alone_ms"] = round(solver_ms(n, p["first"], reps=5, warmup=1)["env_ms"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
