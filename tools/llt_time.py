#!/usr/bin/env python3
"""Times of the tiled Cholesky solve and of the bundle adjustment built on it.  One JSON line per measurement.

  solver   orbm_llt_solve_dev alone at n = 384, 768, 1,536 and 3,072 on B B^T + n I: device events around each call (the matrix is
           restored by a device copy outside the events), median and spread over --reps calls after --warmup.
  ba       orbm_global_bundle_adjustment, the global BA behind a loop closure (10 iterations, keyframe 0 fixed), at 64, 128, 256 and
           512 keyframes with 5 points per keyframe and 3 .. 8 observations per point, and one denser scene (256 keyframes, 20 points
           per keyframe): host clock around whole calls (each ends in its own waits), median of batches, and the time per trial.  At
           64 keyframes orbm_bundle_adjustment (the one-workgroup solve) runs on the same graph in alternating batches.

--profile: kernel times from `rocprofv3 --kernel-trace --stats` in passes of their own (a fresh child process per scene): every
k_llt_* / k_ba_* kernel with calls, mean and share of the kernel time, for the solver at each n and for both entries at 64
keyframes (k_ba_solve against the k_llt_* kernels of one trial) and the new entry at 512."""
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

import ba_scenes                              # noqa: E402
from orb_slam2_e_amd import bundle            # noqa: E402

SOLVER_N = [384, 768, 1536, 3072]
BA_SCENES = [(64, 5), (128, 5), (256, 5), (512, 5), (256, 20)]       # (keyframes, points per keyframe)


def ba_scene(nkf, ppk):
    return ba_scenes.make(nfree=nkf, nfixed=0, npoints=ppk * nkf, seed=6000 + nkf + ppk, kf0_fixed=True, obs_per_point=(3, 8))


def time_solver(n, reps, warmup):
    import torch
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n))
    A = B @ B.T + n * np.eye(n)
    S0 = torch.from_numpy(np.ascontiguousarray(np.tril(A).T)).cuda()
    S = torch.empty_like(S0)
    b = torch.from_numpy(rng.standard_normal(n)).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda"); ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = []
    for k in range(warmup + reps):
        S.copy_(S0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bundle.llt_solve_device(S, b, x, ok)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    assert int(ok.item()) == 1
    T = bundle.llt_tile()
    flops = n ** 3 / 3 * 2                                     # one multiply and one add per term of every dot
    med = float(np.median(ms))
    return {"what": "solver", "n": n, "tile": T, "launches": 4 * ((n + T - 1) // T) - 1, "ms": round(med, 4), "spread_ms": [round(min(ms), 4), round(max(ms), 4)],
            "reps": reps, "gflops_f64_mul_add": round(flops / med / 1e6, 1)}


def batches(fn, nb, calls):
    out = []
    for _ in range(nb):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return out


def time_ba(nkf, ppk, nb, calls):
    g = ba_scene(nkf, ppk)
    opt = bundle.global_options(10, False)
    entries = [("global", bundle.run_global)] + ([("one_workgroup", bundle.run)] if nkf <= 64 else [])
    got = {name: fn(g, opt, want_stats=True) for name, fn in entries}
    for name, fn in entries:
        for _ in range(2):
            fn(g, opt)
    t = {name: [] for name, _ in entries}
    for _ in range(nb):                                        # alternating batches: the same noise for both entries
        for name, fn in entries:
            t[name] += batches(lambda: fn(g, opt), 1, calls)
    line = {"what": "ba", "keyframes": nkf, "points": ppk * nkf, "nedges": int(len(g["e_point"])), "n": 6 * (nkf - 1),
            "trials": got["global"]["trials"], "batches": nb, "calls_per_batch": calls}
    ntr = max(sum(got["global"]["trials"]), 1)
    for name, _ in entries:
        med = float(np.median(t[name]))
        line[name] = {"call_ms": round(med, 3), "spread_ms": [round(min(t[name]), 3), round(max(t[name]), 3)], "ms_per_trial": round(med / ntr, 3)}
    if len(entries) == 2:
        line["same_bytes"] = bool(all(got["global"][k].tobytes() == got["one_workgroup"][k].tobytes() for k in ("poses_d", "points_d", "chi2", "trial_log")))
    return line


def profile(child_args, label):
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "llt", "--output-format", "csv", "--",
                               sys.executable, os.path.abspath(__file__)] + child_args, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                k = re.search(r"k_llt_\w+|k_ba_\w+|k_stage_copy", row.get("Name", ""))
                if k:
                    rows.append((k.group(0), int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["TotalDurationNs"])))
    total = sum(r[3] for r in rows) or 1.0
    line = dict(label)
    line["kernel_ms_total"] = round(total / 1e6, 3)
    line["kernels"] = {k: {"calls": c, "mean_us": round(us, 2), "total_ms": round(t / 1e6, 3), "share": round(t / total, 4)} for k, c, us, t in sorted(rows, key=lambda r: -r[3])}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", default=None, help="(internal) solver,N | ba,ENTRY,KEYFRAMES,POINTS_PER_KEYFRAME: the profiled work alone")
    a = ap.parse_args()
    if a.child:
        w = a.child.split(",")
        if w[0] == "solver":
            time_solver(int(w[1]), 3, 1)
        else:
            g = ba_scene(int(w[2]), int(w[3]))
            for _ in range(2):
                (bundle.run_global if w[1] == "global" else bundle.run)(g, bundle.global_options(10, False))
        return
    if a.profile:
        for n in SOLVER_N:
            profile(["--child", f"solver,{n}"], {"what": "solver_kernels", "n": n, "calls_profiled": 4})
        for entry, nkf in (("one_workgroup", 64), ("global", 64), ("global", 512)):
            profile(["--child", f"ba,{entry},{nkf},5"], {"what": "ba_kernels", "entry": entry, "keyframes": nkf, "calls_profiled": 2})
        return
    for n in SOLVER_N:
        print(json.dumps(time_solver(n, a.reps, a.warmup)), flush=True)
    for nkf, ppk in BA_SCENES:
        print(json.dumps(time_ba(nkf, ppk, a.batches, a.calls)), flush=True)


if __name__ == "__main__":
    main()
