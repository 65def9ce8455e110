#!/usr/bin/env python3
"""Call time of the bundle of Optimizer::PoseOptimizationNR on the closed-loop scenes `median`, `p90` and `large`
(tests/test_cpu_pose_nr_bundle.py): the one-launch call orbm_pose_optimization_nr from Python, and beside it the host-driven form it
replaces -- orbslam_hip::PoseOptimizationNR_fem over the mini-g2o graph with one fem_trial_energy call per Levenberg trial
(tools/cxx/pose_nr_host_loop_time.cpp, built here).  A figure is the median over batches of the mean of 10 calls, with the spread
(min .. max over batches) beside it.  Prints one JSON line per scene.

--scene NAME: that scene only.
--profile: the kernel alone, per scene, each from a `rocprofv3 --kernel-trace --stats` pass of its own (a fresh child process runs
that scene's device call with 3 batches under the profiler; times under the profiler are longer than the call times above)."""
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

import pose_nr_bundle_oracle as nrb                                       # noqa: E402
from orb_slam2_e_amd import pose_optimization_nr                         # noqa: E402
from orb_slam2_e_amd.fem import FEA2, FEM_C3D6, extrude_elems, second_layer    # noqa: E402
from pose_nr_scene import write_scene                                     # noqa: E402

SCENES = [("median", 1), ("p90", 2), ("large", 5)]


def batches(fn, nb, calls):
    out = []
    for _ in range(nb):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return out


def fig(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--scene", choices=[n for n, _ in SCENES])
    a = ap.parse_args()
    scenes = [sc for sc in SCENES if a.scene in (None, sc[0])]
    if a.profile:
        for name, _ in scenes:
            with tempfile.TemporaryDirectory() as d:
                subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "posenr", "--output-format", "csv", "--",
                                       sys.executable, os.path.abspath(__file__), "--batches", "3", "--no-host-loop", "--scene", name],
                                      stdout=subprocess.DEVNULL)
                for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        if "k_pose_nr" in row.get("Name", ""):
                            print(json.dumps({"scene": name, "kernel": "k_pose_nr", "calls": int(row["Calls"]),
                                              "mean_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                              "max_us": round(float(row["MaxNs"]) / 1e3, 2)}), flush=True)
        return
    exe = None
    if not a.no_host_loop:
        exe = os.path.join(tempfile.mkdtemp(), "pose_nr_host_loop_time")
        libdir = os.path.join(ROOT, "orb_slam2_e_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "cxx", "pose_nr_host_loop_time.cpp"), "-o", exe, "-L", libdir, "-lorbslam_hip",
                               f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    for name, seed in scenes:
        top, tris, g, sc, _, u0, ids = nrb.fixture_problem(name, seed)
        ntop = len(top)
        fea = FEA2(second_layer(top, 0.5), extrude_elems(tris, ntop), FEM_C3D6)
        fea.MatrixAssembly()
        fea.ImposeDirichletEncastre_K(ids)
        fea.trial_setup(u0, ids, len(g["points"]))
        ntr = pose_optimization_nr(fea, g, want_stats=True)[4]["ntrials"]
        pose_optimization_nr(fea, g)
        rec = {"scene": name, "points": len(g["points"]), "edges": len(g["e_point"]), "Ksize": 6 * ntop, "trials": int(ntr),
               "one_launch": fig(batches(lambda: pose_optimization_nr(fea, g), a.batches, a.calls))}
        if exe:
            with tempfile.TemporaryDirectory() as d:
                sp = os.path.join(d, "scene.bin")
                write_scene(sp, 2, top, tris, np.zeros((0, 4), np.int32), sc)
                w = subprocess.check_output([exe, sp, str(a.batches), str(a.calls)], timeout=600).split()
            rec["host_loop"] = fig([float(x) for x in w[:-1]])
            rec["host_loop_trials"] = int(w[-1])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
