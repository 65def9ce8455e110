"""What tests/test_cpu_ba.py, tests/test_gpu_ba.py and tests/fuzz_ba.py share: the integer outputs of a bundle-adjustment result, the
relative differences of its continuous ones, and the sensitivity measurement on the restatement alone (test infrastructure)."""
import json
import os

import numpy as np

import ba_oracle
import ba_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_sensitivity.json")
ULP_SEEDS = [7919 * (k + 1) for k in range(16)]
M = 8                   # the project's margin: tolerances are M times the restatement's own sensitivity
RHO_FLOOR = 1e-9
D_EACH = {}             # filled by measure_sensitivity: the restatement's sensitivity in the entry-by-entry measures of diffs_each
CAP = 0.02              # at most 2 % of the scenes may sit at the rounding floor


def ints(r):
    """every integer output: levels, erase, not_included, iterations, trials, results, stopped"""
    return (r["level"].tobytes(), r["erase"].tobytes(), r["not_included"].tobytes(), tuple(r["iterations"]), tuple(r["trials"]),
            tuple(r["results"]), int(r["stopped"]))


def rel(a, b):
    """largest difference over the largest magnitude of the reference b"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def rel_each(a, b, floor):
    """largest per-entry difference over max(|b entry|, floor): every entry is held to the margin on its own scale"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


def diffs(a, b):
    """relative differences of poses (q, t), points, stored chi2 and the trials' lambda and chi2 of result a to reference b, each over
    the largest magnitude of its array: the measure D_cpu was taken with"""
    nt = min(len(a["trial_log"]), len(b["trial_log"]))
    la, lb = a["trial_log"][:nt], b["trial_log"][:nt]
    ok = lb["ok2"] != 0
    return {"poses": rel(a["poses_d"], b["poses_d"]), "points": rel(a["points_d"], b["points_d"]), "chi2": rel(a["chi2"], b["chi2"]),
            "lambda": rel(la["lam"], lb["lam"]), "tempChi": rel(la["tempChi"][ok], lb["tempChi"][ok]),
            "currentChi": rel(la["currentChi"], lb["currentChi"])}


def diffs_each(a, b):
    """The same quantities ENTRY BY ENTRY.  The stored chi2 edge by edge over max(chi2, 1): its thresholds are 5.99 .. 7.815, so 1 is
    the scale on which an ordinary edge's decision is made, and a 40-px outlier's chi2 of thousands does not loosen the others'
    margin.  Lambda trial by trial over its own value, the chi2 sums over max(value, 1).  Held to M times the restatement's own
    sensitivity in the SAME measure (D_each of measure_sensitivity): lambda is multiplied by 1 - (2 rho - 1)^3 at every accepted
    trial and follows the last bits of rho far more closely than the estimates do."""
    nt = min(len(a["trial_log"]), len(b["trial_log"]))
    la, lb = a["trial_log"][:nt], b["trial_log"][:nt]
    ok = lb["ok2"] != 0
    return {"chi2": rel_each(a["chi2"], b["chi2"], 1.0), "lambda": rel_each(la["lam"], lb["lam"], 1e-300),
            "tempChi": rel_each(la["tempChi"][ok], lb["tempChi"][ok], 1.0), "currentChi": rel_each(la["currentChi"], lb["currentChi"], 1.0)}


def thresholds(g, opt):
    """the chi2 threshold of every edge"""
    return np.where(g["e_obs"][:, 2] < 0, opt.chi2_mono, opt.chi2_stereo)


def measure_sensitivity(scenes=None):
    """Every scene under the +-1 ulp switch with 16 seeds, on the restatement ALONE.  d = the largest relative difference of the
    final poses and points to the unperturbed run, D = the largest d.  Per scene also what puts it at the rounding floor: a trial
    with |rho| below 1e-9, a stored chi2 within M D of its threshold (relative), integers that change under a pattern."""
    rows, D = [], 0.0
    D_EACH.clear()
    for name, g, opt in (scenes if scenes is not None else ba_scenes.scenes()):
        base = ba_oracle.run(g, opt)
        d, moved = 0.0, 0
        for seed in ULP_SEEDS:
            o = ba_oracle.run(g, opt, ulp_seed=seed)
            d = max(d, rel(o["poses_d"], base["poses_d"]), rel(o["points_d"], base["points_d"]))
            moved += ints(o) != ints(base)
            if ints(o) == ints(base):
                for k, v in diffs_each(o, base).items():
                    D_EACH[k] = max(D_EACH.get(k, 0.0), v)
        rows.append(dict(name=name, d=d, moved=moved, base=base, g=g, opt=opt))
        D = max(D, d)
    for r in rows:
        th = thresholds(r["g"], r["opt"])
        r["near"] = int(np.sum(np.abs(r["base"]["chi2"] - th) < M * D * th)) if r["opt"].classify else 0
        log = r["base"]["trial_log"]
        r["small_rho"] = int(np.sum(np.abs(log["rho"]) < RHO_FLOOR))
    return D, rows


def write_golden():
    D, rows = measure_sensitivity()
    json.dump({"note": "tests/ba_compare.py measure_sensitivity(): the restatement tests/ba_oracle.c under its +-1 ulp switch, 16 seeds per "
                       "scene; d = largest relative difference of the final poses and points to the unperturbed run; D_cpu = the largest d; D_each = the same runs in the entry-by-entry measures of diffs_each (stored chi2, lambda, the chi2 sums)",
               "D_cpu": D, "D_each": dict(D_EACH), "ulp_seeds": ULP_SEEDS, "scenes": [r["name"] for r in rows], "d": {r["name"]: r["d"] for r in rows}},
              open(GOLDEN, "w"), indent=1)
    return D, rows


if __name__ == "__main__":
    D, rows = write_golden()
    print("D_cpu %.3e" % D)
    for r in rows:
        print("%-22s d %.3e moved %d near %d small_rho %d" % (r["name"], r["d"], r["moved"], r["near"], r["small_rho"]))
