"""What orbm_refine_sim3_candidates computes for one attempt of tests/refine_sim3_scenes.py, as a composition of pieces that exist
without it: SearchBySim3 -> the correspondence walk of Optimizer::OptimizeSim3 (src/Optimizer.cc:1483-1520) in plain numpy ->
OptimizeSim3.  restatement() composes the CPU restatements (oracle.search_by_sim3_whole, tests/sim3_opt_oracle.py); the GPU test
composes the two existing device calls around the same walk."""
import numpy as np

import refine_sim3_scenes as scenes


def already_matched(att):
    """valid1 / valid2 with vbAlreadyMatched1 / 2 of src/ORBmatcher.cc:1333-1343 folded in, as orbm_search_by_sim3 takes them"""
    fam, seed = att["family"], att["seed12"]
    v1, v2 = fam["valid1"].copy(), att["valid2"].copy()
    v1[seed != -1] = 0
    v2[seed[seed >= 0]] = 0
    return v1, v2


def gather(att, found12):
    """Optimizer.cc:1483-1520: for i1 ascending, the pair (i1, i2 = the seed, else what the search found) is a correspondence iff
    i2 >= 0 and both map points are valid.  Returns (a problem dict of tests/sim3_opt_scenes.py's form, vnIndexEdge)."""
    fam, seed = att["family"], att["seed12"]
    merged = np.where(seed >= 0, seed, found12)
    idx, i2s = [], []
    for i1 in range(fam["n1"]):
        i2 = int(merged[i1])
        if i2 < 0 or not fam["valid1"][i1] or not att["valid2"][i2]:
            continue
        idx.append(i1); i2s.append(i2)
    idx, i2s = np.array(idx, np.int64), np.array(i2s, np.int64)
    k1, k2 = fam["kps1"], att["kps2"]
    xy = lambda k, i: np.stack([k["x"][i], k["y"][i]], 1).astype(np.float32).reshape(-1, 2)
    prob = dict(name=att["name"], n=len(idx), fix_scale=fam["fix_scale"], X1w=fam["pos1"][idx].reshape(-1, 3), X2w=att["pos2"][i2s].reshape(-1, 3),
                obs1=xy(k1, idx), obs2=xy(k2, i2s), octave1=k1["octave"][idx].astype(np.int32), octave2=k2["octave"][i2s].astype(np.int32),
                Tcw1=scenes.T1W, Tcw2=att["T2w"], cam1=scenes.CAM, cam2=scenes.CAM, R12=att["R12"], t12=att["t12"], s12=att["s12"],
                th2=np.float32(scenes.TH2))
    return prob, idx


def scatter(att, found12, idx, kept):
    """vpMatches1 as OptimizeSim3 leaves it: the merged index, -1 where the cut erased it (:1577-1590 / :1611-1620); -2 stays"""
    seed = att["seed12"]
    m = np.where(seed == -1, found12, seed).astype(np.int32)
    m[idx[~np.asarray(kept, bool)]] = -1
    return m


def cpu_search(att):
    """oracle.search_by_sim3_whole on the attempt: (found12, nfound)"""
    import oracle
    fam = att["family"]
    if att["n2"] == 0:
        return np.full(fam["n1"], -1, np.int32), 0
    v1, v2 = already_matched(att)
    r = oracle.search_by_sim3_whole(fam["kps1"], fam["desc1"], att["kps2"], att["desc2"], scenes.BOUNDS, scenes.CAM, scenes.SF, scenes.LOG_SF,
                                    scenes.T1W, att["T2w"], att["s12"], att["R12"], att["t12"], v1, fam["pos1"], fam["mind1"], fam["maxd1"],
                                    fam["mp_desc"], v2, att["pos2"], att["mind2"], att["maxd2"], att["mp_desc2"], scenes.TH, scenes.TH_HIGH)
    return r[0], int(r[1])


def restatement(att, ulp_seed=0):
    """dict(found12, nfound, matches12, problem, idx, opt = tests/sim3_opt_oracle.optimize's dict)"""
    import sim3_opt_oracle as so
    found, nf = cpu_search(att)
    prob, idx = gather(att, found)
    opt = so.optimize(prob, scenes.INV_SIGMA2, ulp_seed=ulp_seed)
    return dict(found12=found, nfound=nf, matches12=scatter(att, found, idx, opt["kept"]), problem=prob, idx=idx, opt=opt)
