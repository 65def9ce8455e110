"""What tests/test_cpu_essential_graph.py and tests/test_gpu_essential_graph.py share: the integer outputs of an essential-graph
result, the relative differences of its continuous ones, and the sensitivity measurement on the restatement alone (test
infrastructure).  The method is tests/ba_compare.py's: D = the restatement's own sensitivity to the last bit of
sin / cos / acos / log / exp, the margin M = 8 D, scenes selected off the rounding floor.  A pose graph converges in a few iterations
and then sits at the floor, where the sign of rho is rounding: every scene is therefore measured in two forms, form 1 with the few
iterations of essential_graph_scenes.ITER1 (integers compared) and form 2 with the reference's 20 (continuous outputs only)."""
import json
import os

import numpy as np

import essential_graph_oracle as oracle
import essential_graph_scenes as scenes_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eg_sensitivity.json")
ULP_SEEDS = [7919 * (k + 1) for k in range(16)]
M = 8
RHO_FLOOR = 1e-9
CAP = 0.02              # at most 2 % of the scenes may sit at the rounding floor
D_EACH = {}


def ints(r):
    """every integer output: iterations, trials, results, and the trial log's accepted / ok2 / qmax"""
    log = r["trial_log"]
    return (int(r["iterations"]), int(r["trials"]), tuple(r["results"]), log["accepted"].tobytes(), log["ok2"].tobytes(), log["qmax"].tobytes())


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def rel_each(a, b, floor):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


def diffs_final(a, b):
    """estimates, poses and points of result a against reference b, each over the largest magnitude of its array"""
    return {"estimates": rel(a["estimates"], b["estimates"]), "poses": rel(a["poses"], b["poses"]), "points": rel(a["points"], b["points"])}


def diffs(a, b):
    """the same plus stored chi2, lambda and the trials' chi2 (form 1: the trial logs have the same length)"""
    la, lb = a["trial_log"], b["trial_log"]
    ok = lb["ok2"] != 0
    d = diffs_final(a, b)
    d.update(chi2=rel(a["chi2"], b["chi2"]), **{"lambda": rel(la["lam"], lb["lam"])}, tempChi=rel(la["tempChi"][ok], lb["tempChi"][ok]),
             currentChi=rel(la["currentChi"], lb["currentChi"]))
    return d


def chi_floor(b):
    """the scale on which a chi2 entry is held: an edge's chi2 falls to 1e-30 where the graph is consistent, and its differences are
    those of the sum it was part of -- the reference's chi2 at the start, which the first trial gives back as rho * scale + tempChi"""
    log = b["trial_log"]
    return max(float(log["rho"][0] * log["scale"][0] + log["tempChi"][0]) if len(log) else 0.0, 1e-300)


def diffs_each(a, b):
    """ENTRY BY ENTRY, as tests/ba_compare.py: the stored chi2 edge by edge and the chi2 sums over max(value, the scene's chi2 scale),
    lambda trial by trial over its own value"""
    la, lb = a["trial_log"], b["trial_log"]
    ok = lb["ok2"] != 0
    f = chi_floor(b)
    return {"chi2": rel_each(a["chi2"], b["chi2"], f), "lambda": rel_each(la["lam"], lb["lam"], 1e-300),
            "tempChi": rel_each(la["tempChi"][ok], lb["tempChi"][ok], f), "currentChi": rel_each(la["currentChi"], lb["currentChi"], f)}


def measure_sensitivity(names=None):
    """Every scene in both forms under the +-1 ulp switch with 16 seeds, on the restatement ALONE.  d = the largest relative
    difference of the final estimates, poses and points to the unperturbed run, D = the largest d over the scenes and forms.  Form 1
    also gives what puts a scene at the rounding floor: a trial with |rho| below 1e-9, integers that change under a pattern."""
    rows, D = [], 0.0
    D_EACH.clear()
    for name, g in scenes_mod.scenes(names):
        it1 = scenes_mod.ITER1[name]
        base1, base2 = oracle.run(g, it1), oracle.run(g, scenes_mod.ITER2)
        d1 = d2 = 0.0
        moved = 0
        for seed in ULP_SEEDS:
            o1, o2 = oracle.run(g, it1, ulp_seed=seed), oracle.run(g, scenes_mod.ITER2, ulp_seed=seed)
            d2 = max(d2, *diffs_final(o2, base2).values())
            same = ints(o1) == ints(base1)
            moved += not same
            if same:
                d1 = max(d1, *diffs_final(o1, base1).values())
                for k, v in diffs_each(o1, base1).items():
                    D_EACH[k] = max(D_EACH.get(k, 0.0), v)
        small = int(np.sum(np.abs(base1["trial_log"]["rho"]) < RHO_FLOOR))
        rows.append(dict(name=name, d1=d1, d2=d2, moved=moved, small_rho=small, base1=base1, base2=base2))
        D = max(D, d1, d2)
    return D, rows


def write_golden():
    D, rows = measure_sensitivity()
    json.dump({"note": "tests/essential_graph_compare.py measure_sensitivity(): the restatement tests/essential_graph_oracle.c under its +-1 ulp "
                       "switch, 16 seeds per scene and form; d1 / d2 = largest relative difference of the final estimates, poses and points to "
                       "the unperturbed run with ITER1 / 20 iterations; D_cpu = the largest of them; D_each = the form-1 runs in the "
                       "entry-by-entry measures of diffs_each (stored chi2, lambda, the chi2 sums)",
               "D_cpu": D, "D_each": dict(D_EACH), "ulp_seeds": ULP_SEEDS, "scenes": [r["name"] for r in rows],
               "iter1": {r["name"]: scenes_mod.ITER1[r["name"]] for r in rows}, "d1": {r["name"]: r["d1"] for r in rows},
               "d2": {r["name"]: r["d2"] for r in rows}}, open(GOLDEN, "w"), indent=1)
    return D, rows


if __name__ == "__main__":
    D, rows = write_golden()
    print("D_cpu %.3e" % D, {k: "%.3e" % v for k, v in D_EACH.items()})
    for r in rows:
        print("%-18s d1 %.3e d2 %.3e moved %d small_rho %d  it %d tr %d %s" % (r["name"], r["d1"], r["d2"], r["moved"], r["small_rho"],
              r["base1"]["iterations"], r["base1"]["trials"], r["base1"]["results"]))
