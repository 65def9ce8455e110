#!/usr/bin/env python3
"""Fuzzer for orbm_pnp_hypotheses: random problems -- sizes, outlier shares, poses, minimal-inlier settings, carried bests, sets
drawn with either draw rule (the fork's repeats correspondences), degenerate sets mixed in -- device against the literal
restatement (tests/pnp_oracle.c), bit for bit as tests/test_gpu_pnp.py compares.  Run by hand on a machine with a device:
    python tests/fuzz_pnp.py [--seconds 60] [--seed 1]
Not part of the suite."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pnp_scenes as scenes                  # noqa: E402
import test_gpu_pnp as gpu                   # noqa: E402
from orb_slam2_e_amd import pnp              # noqa: E402


def random_problem(rng, k):
    n = int(rng.choice([4, 5, 7, 20, 63, 64, 65, 130, 300, int(rng.integers(4, 700))]))
    H = int(rng.choice([0, 1, 5, 64, int(rng.integers(1, 301))]))
    axis = rng.standard_normal(3)
    p = scenes.problem(int(rng.integers(1 << 30)), n, H, outliers=float(rng.uniform(0, 0.7)) if n > 4 else 0.0, axis=axis, deg=float(rng.uniform(-90, 90)),
                       t=rng.uniform(-1, 1, 3), min_inliers=int(rng.integers(1, max(2, n))), frame_rule=bool(rng.integers(2)), name=f"fuzz{k}")
    if H >= 8 and n >= 30 and rng.random() < 0.3:
        Xw, uv, octave, sets = scenes.degenerate_sets(p, rng)
        p = dict(p, n=len(Xw), Xw=Xw, uv=uv, octave=octave, sets=np.concatenate([p["sets"][:H - 8], sets]))
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    t0, calls, hyps = time.time(), 0, 0
    while time.time() - t0 < a.seconds:
        probs = [random_problem(rng, calls * 100 + k) for k in range(int(rng.integers(1, 6)))]
        best = [int(rng.integers(-2, p["n"] + 2)) for p in probs]
        res = pnp.pnp_hypotheses([gpu._c(p) for p in probs], scenes.SIGMA2, best)
        for p, r, b in zip(probs, res, best):
            gpu._assert_equal(p, r, b)
            hyps += p["H"]
        calls += 1
    print(f"fuzz_pnp: {calls} calls, {hyps} hypotheses, device == restatement bit for bit (seed {a.seed})")


if __name__ == "__main__":
    main()
