#!/usr/bin/env python3
"""Random graphs through orbm_bundle_adjustment against the CPU restatement (tests/ba_oracle.c).  Run by hand on the MI355X, not
collected by pytest:  python tests/fuzz_ba.py [--n 200] [--seed 1]
A graph whose restatement run sits at the rounding floor (a trial with |rho| < 1e-9, a stored chi2 within M D_cpu of its threshold)
is compared on its continuous outputs only when the integers agree; every other graph must agree on every integer and within
M D_cpu = 8 times the pinned sensitivity."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ba_compare                             # noqa: E402
import ba_oracle                              # noqa: E402
import ba_scenes                              # noqa: E402
from orb_slam2_e_amd import bundle            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    D = json.load(open(ba_compare.GOLDEN))["D_cpu"]
    rng = np.random.default_rng(a.seed)
    worst, floor, bad = 0.0, 0, 0
    for k in range(a.n):
        nfree = int(rng.choice([1, 2, 3, 5, 11, 20, 64]))
        kw = dict(nfree=nfree, nfixed=int(rng.integers(0 if nfree > 1 else 1, 6)), npoints=int(rng.integers(12, 400)), seed=int(rng.integers(1 << 30)),
                  mode=str(rng.choice(["mono", "stereo", "mixed"])), outlier_edges=int(rng.integers(0, 4)), kf0_fixed=bool(rng.random() < 0.3 and nfree > 1),
                  behind=bool(rng.random() < 0.2), single_mono=bool(rng.random() < 0.2), lonely_points=int(rng.integers(0, 3)))
        g = ba_scenes.make(**kw)
        opt = bundle.local_options() if rng.random() < 0.7 else bundle.global_options(int(rng.integers(1, 21)), bool(rng.random() < 0.5))
        r = ba_oracle.run(g, opt)
        d = bundle.run(g, opt, want_stats=True)
        th = ba_compare.thresholds(g, opt)
        at_floor = bool((np.abs(r["trial_log"]["rho"]) < ba_compare.RHO_FLOOR).any() or
                        (opt.classify and (np.abs(r["chi2"] - th) < ba_compare.M * D * th).any()))
        same = ba_compare.ints(d) == ba_compare.ints(r)
        floor += at_floor
        if not same and not at_floor:
            bad += 1
            print("INTEGERS DIFFER", kw, flush=True)
        if same:
            v = max(ba_compare.diffs(d, r).values())
            worst = max(worst, v)
            if v > ba_compare.M * D and not at_floor:
                bad += 1
                print("DIFFERENCE %.3e" % v, kw, flush=True)
    print(json.dumps({"graphs": a.n, "at_the_floor": floor, "failures": bad, "largest_difference": worst, "M_D_cpu": ba_compare.M * D}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
