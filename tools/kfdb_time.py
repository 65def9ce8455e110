#!/usr/bin/env python3
"""Call time of the keyframe database on the device against the reference's database on one CPU thread of the same box:
  orbm_kfdb_query   one query of ~1,500 words against K = 100, 1,000, 5,000, 20,000 keyframes of ~1,500 words each, over a vocabulary
                    of ORBvoc's size (971,000 words);
  orbm_kfdb_add     one keyframe's row;
  orbm_kfdb_score   20 slots (LoopClosing::DetectLoop's minScore loop);
against tests/kfdb_oracle.cc built -O3 -march=native, pinned to one CPU and fed the same rows (a binary file) and the same query:
its DetectRelocalizationCandidates (the walk over the inverted file, the scores of the keyframes that pass the word cut, the fold),
its add and its score loop.  The capability is new, so there is no parent-commit figure: the CPU restatement is the yardstick.
The like-for-like figure beside it is detect_cxx_ms: orbslam_hip::KeyFrameDatabase::DetectRelocalizationCandidates from C++
(tests/cxx/kfdb_host.cpp built -O2), the query call PLUS the host half (the scan of the K slots, the sort of the sharing ones, the
cut and the fold), median of the same number of runs on the same rows and query.

Keyframes belong to places of 20: a keyframe takes 60 % of its words from its place's pool of 3,000 and the rest from the whole
vocabulary; the query is of place 0 at 90 %.  About 20 keyframes therefore share hundreds of words with the query and every other
one a handful, which is what the reference's inverted file is good at.

The device calls go through bare ctypes with preallocated rows; a figure is the median over batches of the mean of --calls calls,
with the spread (min .. max over batches) beside it.  The device's scores are compared with the oracle's, bit for bit, before
anything is timed.  Prints one JSON line per K."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import kfdb_scenes as S                                            # noqa: E402
from orb_slam2_e_amd._lib import lib, ptr as _p                    # noqa: E402

NWORDS = 971000


def row(rng, pool, n, share):
    k = min(int(share * n), len(pool))
    words = np.unique(np.concatenate([rng.choice(pool, k, replace=False), rng.integers(0, NWORDS, n - k)])).astype(np.int32)
    v = rng.uniform(0.05, 4.0, len(words))
    return words, v / v.sum()


def median_ms(fn, batches, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ts.append((time.perf_counter() - t0) / calls * 1e3)
    return round(float(np.median(ts)), 4), [round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 5000, 20000])
    ap.add_argument("--words", type=int, default=1500)
    ap.add_argument("--cpu", type=int, default=None, help="the CPU the oracle is pinned to (default: the last one this process may use)")
    a = ap.parse_args()
    L = lib()
    cpu = a.cpu if a.cpu is not None else max(os.sched_getaffinity(0))
    tmp = tempfile.mkdtemp(prefix="kfdb_time_")
    exe = S.build_oracle(tmp, flags=("-O3", "-march=native"))
    host = os.path.join(tmp, "kfdb_host")
    libdir = os.path.join(ROOT, "orb_slam2_e_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "kfdb_host.cpp"),
                           "-o", host, "-L", libdir, "-lorbslam_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    for K in a.keyframes:
        rng = np.random.default_rng(K)
        pools = [np.unique(rng.integers(0, NWORDS, 3000)) for _ in range(max(K // 20, 1))]
        rows = [row(rng, pools[k // 20 % len(pools)], a.words, 0.6) for k in range(K)]
        qw, qv = row(rng, pools[0], a.words, 0.9)
        h = C.c_void_p()
        assert L.orbm_kfdb_create(NWORDS, C.byref(h)) == 0
        slot = C.c_int(0)
        t_add = []
        for k0 in range(0, K, 100):                                # adds in batches of 100
            t0 = time.perf_counter()
            for w, v in rows[k0:k0 + 100]:
                assert L.orbm_kfdb_add(h, _p(w), _p(v), len(w), C.byref(slot)) == 0
            t_add.append((time.perf_counter() - t0) / len(rows[k0:k0 + 100]) * 1e3)
        common, first, score = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.float32)
        pq = (_p(qw), _p(qv), len(qw), _p(common), _p(first), _p(score))
        query = lambda: L.orbm_kfdb_query(h, *pq)
        assert query() == 0
        waits = L.orbm_debug_last_kfdb_waits()
        slots20 = np.arange(0, 20, dtype=np.int32) % K
        out20 = np.zeros(20, np.float32)
        ps = (_p(qw), _p(qv), len(qw), _p(slots20), 20, _p(out20))
        score20 = lambda: L.orbm_kfdb_score(h, *ps)
        assert score20() == 0
        # the same case on the CPU: rows as a binary file, the query as text
        path = os.path.join(tmp, f"rows_{K}.bin")
        with open(path, "wb") as f:
            f.write(np.int32(K).tobytes())
            for w, v in rows:
                f.write(np.int32(len(w)).tobytes()); f.write(w.tobytes()); f.write(v.astype(np.float64).tobytes())
        bow = " ".join([str(len(qw))] + [f"{int(w)} {float(v).hex()}" for w, v in zip(qw, qv)])
        reps = a.batches * a.calls
        case = os.path.join(tmp, f"case_{K}.txt")
        with open(case, "w") as f:
            f.write(f"N {NWORDS}\nB {path}\nQ {bow}\nTR {reps} {bow}\nTS {reps} 20 " + " ".join(map(str, slots20)) + f" {bow}\n")
        cp = subprocess.run([exe, case], capture_output=True, text=True, check=True, preexec_fn=lambda: os.sched_setaffinity(0, {cpu}))
        lines = cp.stdout.split("\n")
        cpu_add_us = float(lines[0].split()[2])
        ref = [ln.split() for ln in lines[2:2 + K]]
        assert np.array_equal(common, [int(r[0]) for r in ref]) and np.array_equal(first, [int(r[1]) for r in ref])
        assert S.same_bits(score, [np.float32(float.fromhex(r[2])) for r in ref]), "device scores differ from the oracle's"
        cpu_detect_us = float(lines[2 + K].split()[1]); cpu_score_us = float(lines[3 + K].split()[1])
        with open(case, "w") as f:
            f.write(f"N {NWORDS}\nB {path}\nTR {reps} {bow}\n")
        hp = subprocess.run([host, case], capture_output=True, text=True, check=True)
        detect_cxx_us = float(hp.stdout.split("\n")[1].split()[1])
        os.remove(path)
        line = {"keyframes": K, "words": a.words, "nwords": NWORDS, "sharing": int((common > 0).sum()), "max_common": int(common.max()),
                "waits_query": waits, "batches": a.batches, "calls_per_batch": a.calls}
        line["query_ms"], line["query_spread_ms"] = median_ms(query, a.batches, a.calls)
        line["detect_cxx_ms"] = round(detect_cxx_us / 1e3, 4)
        line["cpu_detect_ms"] = round(cpu_detect_us / 1e3, 4)
        line["score20_ms"], line["score20_spread_ms"] = median_ms(score20, a.batches, a.calls)
        line["cpu_score20_ms"] = round(cpu_score_us / 1e3, 4)
        line["add_ms"] = round(float(np.median(t_add)), 4)
        line["add_spread_ms"] = [round(min(t_add), 4), round(max(t_add), 4)]
        line["cpu_add_ms"] = round(cpu_add_us / 1e3, 4)
        print(json.dumps(line), flush=True)
        assert L.orbm_kfdb_destroy(h) == 0


if __name__ == "__main__":
    main()
