"""Differential fuzz of orbm_frame_search_by_bow_pairs vs the literal oracle loop, pair by pair: random K (0 .. 64), random sizes
(down to one keypoint, now and then an empty feature vector), random masks, frames shared between pairs on either side, both
forms, both resolvers, with and without the rotation check.  Not collected by pytest.
usage (GPU box): PYTHONPATH=. python tests/fuzz_bow_pairs.py [batches] [seed]"""
import sys
import numpy as np
import oracle
from orb_slam2_e_amd import KP_DTYPE, Frame, ORBmatcher
from orb_slam2_e_amd._lib import lib
from orb_slam2_e_amd.synth import synth_bow_case

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0; tot = 0; npairs = 0; waits = {}
BOUNDS = (0.0, 0.0, 640.0, 480.0)
EMPTY = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))


def side(d, a, node, keep, valid):
    k = np.zeros(len(d), KP_DTYPE)
    k["x"] = rng.uniform(-10, 650, len(d)); k["y"] = rng.uniform(-10, 490, len(d)); k["angle"] = a        # (some outside the grid)
    fv = EMPTY if rng.random() < 0.05 else oracle.feature_vector(node, keep)
    return dict(frame=Frame(k, d, BOUNDS), fv=fv, valid=valid, desc=d, angle=a)


for case in range(n):
    K = int(rng.choice([0, 1, 2, 3, 5, 8, 13, 33, 64]))
    nbase = int(rng.integers(1, 5))
    firsts, seconds = [], []
    for _ in range(nbase):
        n1 = int(rng.integers(1, 900)); n2 = int(rng.integers(1, 900)); nn = int(rng.integers(1, 60))
        d1, a1, node1, keep1, valid1, d2, a2, node2, keep2, valid2 = synth_bow_case(int(rng.integers(0, 1 << 30)), n1=n1, n2=n2, nnodes=nn)
        firsts.append(side(d1, a1, node1, keep1, valid1)); seconds.append(side(d2, a2, node2, keep2, valid2))
    # a pair takes the two sides of one base (matches), or sides of two bases (few or none); every side serves several pairs
    pairs = []
    for _ in range(K):
        b = int(rng.integers(0, nbase))
        pairs.append((firsts[b], seconds[b if rng.random() < 0.8 else int(rng.integers(0, nbase))]))
    kf = bool(rng.integers(0, 2)); ori = bool(rng.integers(0, 2)); ratio = float(rng.choice([0.6, 0.75, 0.9]))
    seq = int(rng.integers(0, 2))
    lib().orbm_debug_force_sequential_resolver(seq)
    m = ORBmatcher(ratio, ori)
    got = m.frame_search_by_bow_pairs([(a["frame"], a["fv"], a["valid"], b["frame"], b["fv"], b["valid"]) for a, b in pairs], kf)
    w = ORBmatcher.last_bow_pairs_waits()
    waits[w] = waits.get(w, 0) + 1
    for k, ((a, b), g) in enumerate(zip(pairs, got)):
        ref = oracle.search_by_bow(a["fv"], a["valid"], a["desc"], a["angle"], b["fv"], b["valid"] if kf else None, b["desc"], b["angle"], kf, ratio, ori)
        tot += int(ref[2]); npairs += 1
        if not (g[2] == ref[2] and np.array_equal(g[0], ref[0]) and np.array_equal(g[1], ref[1])):
            bad += 1; print("MISMATCH", case, "pair", k, "of", K, kf, ori, ratio, "sequential" if seq else "parallel", flush=True)
    for s in firsts + seconds:
        s["frame"].close()
lib().orbm_debug_force_sequential_resolver(0)
print("batches", n, "pairs", npairs, "mismatches", bad, "matches seen", tot, "host waits seen", dict(sorted(waits.items())))
sys.exit(1 if bad else 0)
