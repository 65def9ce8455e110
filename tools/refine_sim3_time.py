#!/usr/bin/env python3
"""Call time of the refinement tail of LoopClosing::ComputeSim3 for P attempts against one current keyframe, 2000-keypoint keyframes
with about 50 and about 300 correspondences per attempt (a third of them seeds, the start 0.2 degrees / 0.2 % off):
  (a) chained      one orbm_refine_sim3_candidates call over the P attempts;
  (b) singles      P x (orbm_search_by_sim3 + the host walk of Optimizer.cc:1483-1520 + one orbm_optimize_sim3 of one problem);
  (c) batched_opt  the P searches with their host walks, then ONE orbm_optimize_sim3 over the P problems.
All three from this build, through bare ctypes with preallocated outputs and inputs prepared once (the seeds folded into the valid
arrays for (b) / (c)); the host walk is vectorised numpy.  The forms alternate in one process; a figure is the median over batches of
the mean of 10 calls, with the spread (min .. max over batches) beside it.  Prints one JSON line per (correspondences, P); the
outputs of the three forms are compared before anything is timed.

--profile: kernel times from a `rocprofv3 --kernel-trace --stats` pass of its own per shape (a fresh child process runs form (a) with
3 batches under the profiler; times under the profiler are longer than the call times)."""
import argparse
import csv
import ctypes as C
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

import refine_sim3_reference as ref          # noqa: E402
import refine_sim3_scenes as S               # noqa: E402
from orb_slam2_e_amd import Frame, Points, View              # noqa: E402
from orb_slam2_e_amd import sim3 as s3                       # noqa: E402
from orb_slam2_e_amd._lib import lib, ptr as _p              # noqa: E402

N_KP = 2000
SHARED = {50: 75, 300: 420}          # family points KF2 observes, for about that many correspondences
KERNELS = r"k_project_pair_jobs|k_win_best_jobs|k_refine_gather|k_sim3_optimize<\d+>|k_stage_copy"


def f32(a, n):
    return np.ascontiguousarray(a, np.float32).reshape(n)


class Pass:
    """P attempts of one family, every form's arguments built once"""

    def __init__(self, ncorr, P):
        self.L = lib()
        fam = S.family(40 + ncorr, N_KP, spread=0.9)
        self.fam, self.P, self.n1 = fam, P, fam["n1"]
        self.atts = [S.attempt(fam, f"time{k}", 500 + k, shared=SHARED[ncorr], clutter=N_KP - SHARED[ncorr], seeds=0.33) for k in range(P)]
        self.view = View(*S.CAM, 0.08, 40.0, S.LOG_SF, S.SF)
        self.isg, self.T1 = S.INV_SIGMA2, f32(S.T1W, 16)
        self.k1 = Frame(fam["kps1"], fam["desc1"], S.BOUNDS)
        mk = lambda v, pos, d, mn, mx: Points(v, pos, d, min_distance=mn, max_distance=mx)
        self.p1 = mk(fam["valid1"], fam["pos1"], fam["mp_desc"], fam["mind1"], fam["maxd1"])
        self.k2 = [Frame(a["kps2"], a["desc2"], S.BOUNDS) for a in self.atts]
        self.p2 = [mk(a["valid2"], a["pos2"], a["mp_desc2"], a["mind2"], a["maxd2"]) for a in self.atts]
        # (a)
        self.arr = (s3._CRefineSim3Attempt * P)()
        self.found = np.zeros((P, self.n1), np.int32); self.matches = np.zeros((P, self.n1), np.int32)
        self.nf = np.zeros(P, np.int32); self.res = (s3.Sim3OptResult * P)()
        self.keep = []
        for k, (c, a) in enumerate(zip(self.arr, self.atts)):
            T2, R, t, seed = f32(a["T2w"], 16), f32(a["R12"], 9), f32(a["t12"], 3), np.ascontiguousarray(a["seed12"], np.int32)
            self.keep.append((T2, R, t, seed))
            c.kf2, c.points2, c.T2w = self.k2[k]._h.value, C.addressof(self.p2[k].c), _p(T2).value
            c.R12, c.t12, c.s12 = (C.c_float * 9)(*R), (C.c_float * 3)(*t), float(a["s12"])
            c.seed12, c.found12, c.matches12 = _p(seed).value, _p(self.found[k]).value, _p(self.matches[k]).value
        # (b), (c): orbm_search_by_sim3 takes valid with vbAlreadyMatched1 / 2 folded in
        self.folded = []
        for a in self.atts:
            v1, v2 = ref.already_matched(a)
            self.folded.append((mk(v1, fam["pos1"], fam["mp_desc"], fam["mind1"], fam["maxd1"]), mk(v2, a["pos2"], a["mp_desc2"], a["mind2"], a["maxd2"])))
        self.m12 = np.zeros((P, self.n1), np.int32)
        self.xy1 = np.stack([fam["kps1"]["x"], fam["kps1"]["y"]], 1).astype(np.float32); self.oct1 = fam["kps1"]["octave"].astype(np.int32)
        self.xy2 = [np.stack([a["kps2"]["x"], a["kps2"]["y"]], 1).astype(np.float32) for a in self.atts]
        self.oct2 = [a["kps2"]["octave"].astype(np.int32) for a in self.atts]
        self.v1b = fam["valid1"].astype(bool); self.v2b = [a["valid2"].astype(bool) for a in self.atts]
        self.kept = np.zeros(P * self.n1 + 1, np.uint8)
        self.res1 = (s3.Sim3OptResult * P)()

    def chained(self):
        v = self.view
        assert self.L.orbm_refine_sim3_candidates(self.k1._h, C.byref(self.p1.c), _p(self.T1), C.byref(v.c), _p(self.isg), self.arr, self.P,
                                                  S.TH, S.TH_HIGH, S.TH2, 0, _p(self.nf), self.res) == 0
        return [(self.found[k].copy(), int(self.nf[k]), self.matches[k].copy(), bytes(self.res[k])) for k in range(self.P)]

    def _search_and_walk(self, k):
        a, (T2, R, t, seed) = self.atts[k], self.keep[k]
        q1, q2 = self.folded[k]
        nf = C.c_int(0)
        assert self.L.orbm_search_by_sim3(self.k1._h, self.k2[k]._h, C.byref(self.view.c), _p(self.T1), _p(T2), float(a["s12"]), _p(R), _p(t),
                                          C.byref(q1.c), C.byref(q2.c), S.TH, S.TH_HIGH, None, None, _p(self.m12[k]), C.byref(nf), None, None) == 0
        found = self.m12[k]
        merged = np.where(seed >= 0, seed, found)                                   # Optimizer.cc:1483-1520
        idx = np.nonzero((merged >= 0) & self.v1b & self.v2b[k][np.maximum(merged, 0)])[0]
        i2 = merged[idx]
        prob = s3.Sim3OptProblem(self.fam["pos1"][idx], a["pos2"][i2], self.xy1[idx], self.xy2[k][i2], self.oct1[idx], self.oct2[k][i2], S.T1W, T2,
                                 S.CAM, S.CAM, R, t, a["s12"], S.TH2, False)
        return found, nf.value, seed, idx, prob

    def _scatter(self, found, seed, idx, kept):
        m = np.where(seed == -1, found, seed)
        m[idx[kept == 0]] = -1
        return m

    def singles(self):
        out = []
        for k in range(self.P):
            found, nf, seed, idx, prob = self._search_and_walk(k)
            c = prob.c()
            assert self.L.orbm_optimize_sim3(C.byref(c), 1, _p(self.isg), len(self.isg), self.res1, _p(self.kept)) == 0
            out.append((found.copy(), nf, self._scatter(found, seed, idx, self.kept[:prob.n]), bytes(self.res1[0])))
        return out

    def batched_opt(self):
        parts = [self._search_and_walk(k) for k in range(self.P)]
        arr = (s3._CSim3OptProblem * self.P)(*[p[4].c() for p in parts])
        assert self.L.orbm_optimize_sim3(arr, self.P, _p(self.isg), len(self.isg), self.res1, _p(self.kept)) == 0
        out, at = [], 0
        for k, (found, nf, seed, idx, prob) in enumerate(parts):
            out.append((found.copy(), nf, self._scatter(found, seed, idx, self.kept[at:at + prob.n]), bytes(self.res1[k])))
            at += prob.n
        return out


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3] for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shape", default=None, help="correspondences,P: one shape instead of the eight")
    ap.add_argument("--only-chained", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    shapes = [(n, P) for n in (50, 300) for P in (1, 4, 8, 16)] if a.shape is None else [tuple(int(v) for v in a.shape.split(","))]
    if a.profile:
        for n, P in shapes:
            with tempfile.TemporaryDirectory() as d:
                subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "refine", "--output-format", "csv", "--",
                                       sys.executable, os.path.abspath(__file__), "--batches", "3", "--only-chained", "--shape", f"{n},{P}"],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        m = re.search(KERNELS, row.get("Name", ""))
                        if m:
                            print(json.dumps({"kernel": m.group(0), "correspondences": n, "attempts": P, "calls": int(row["Calls"]),
                                              "mean_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                              "max_us": round(float(row["MaxNs"]) / 1e3, 2)}), flush=True)
        return
    for n, P in shapes:
        ps = Pass(n, P)
        forms = [("chained", ps.chained)] + ([] if a.only_chained else [("singles", ps.singles), ("batched_opt", ps.batched_opt)])
        got = ps.chained()
        waits = s3.last_refine_sim3_waits()
        for _, fn in forms[1:]:
            assert same(got, fn()), "the forms differ"
        for _ in range(3):
            for _, fn in forms:
                fn()
        times = {name: [] for name, _ in forms}
        for _ in range(a.batches):
            for name, fn in forms:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                times[name].append((time.perf_counter() - t0) / a.calls * 1e3)
        line = {"keypoints": N_KP, "attempts": P, "correspondences": [int(np.frombuffer(r[3], np.int32, 3, 64)[2]) for r in got],
                "nin": [int(np.frombuffer(r[3], np.int32, 1, 64)[0]) for r in got], "waits_chained": waits, "batches": a.batches,
                "calls_per_batch": a.calls}
        for name, ts in times.items():
            line[name + "_ms"] = round(float(np.median(ts)), 4)
            line[name + "_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
