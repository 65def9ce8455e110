"""Scenes for orbm_global_bundle_adjustment_env (tests/test_cpu_ba_env.py, tests/test_gpu_ba_env.py).  tests/ba_scenes.make
draws a point's observers from ALL keyframes, so its reduced systems are full.  Here covisibility is local in time: the cameras move
along a path past a cloud of points, a point belongs to one keyframe of the path and is observed by 3 .. 8 keyframes inside a window
of +- w around it, and planted `loops` add points observed by a few early AND a few late keyframes.  With the keyframes listed in
path order the Schur complement is a band with a few far blocks.  Everything is held as the floats the reference holds; a scene is
(name, graph, options) as in tests/ba_scenes.py.  The restatement tests/ba_oracle.c has no size limit and is the reference,
unchanged.  Its own sensitivity on the scenes up to e130 is pinned in tests/golden/ba_env_sensitivity.json (the format of
ba_sensitivity.json); e520 takes the restatement about 20 s, so its result is a golden, tests/golden/ba_env_520.npz, with a SHA-256
of the scene's input arrays and its sensitivity under the first 4 ulp patterns.  `python tests/ba_env_scenes.py` rewrites both
(test infrastructure: never part of the product)."""
import json
import os

import numpy as np

import ba_compare
import ba_large_scenes
import ba_oracle
from ba_scenes import BF, CX, CY, FX, FY, _rot
from orb_slam2_e_amd import bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_env_sensitivity.json")
GOLDEN_520 = os.path.join(ROOT, "tests", "golden", "ba_env_520.npz")
STEP = 0.05                     # metres between two keyframes of the path
KEYS_520 = ba_large_scenes.KEYS_512


def make(nfree, seed, nfixed=0, w=4, points_per_kf=5, loops=(), mode="mixed", noise_px=0.5, pose_err=(0.004, 0.02), point_err=0.02,
         kf0_fixed=True, all_outlier_keyframe=None, lonely_points=0, permute=False):
    """The flat graph.  The path holds the nfixed fixed keyframes first, then the free ones, STEP apart; the free keyframes are listed
    in path order (ascending mnId), the fixed ones behind them as orbm_ba_graph wants them.
      w                     a point of keyframe k is observed by 3 .. 8 keyframes of k - w .. k + w
      loops                 ((early_lo, early_hi), (late_lo, late_hi), npoints): that many points more, each observed by EVERY free
                            keyframe of both inclusive ranges
      all_outlier_keyframe  every observation of THAT free keyframe moved by 40 .. 80 px: all its edges go to level 1
      lonely_points         that many points without any edge
      permute               the free keyframes are listed in a random order (the graph is the same, the envelope is not)
    mode, noise_px, pose_err, point_err, kf0_fixed as tests/ba_scenes.make."""
    rng = np.random.default_rng(seed)
    npath = nfixed + nfree
    index = np.concatenate([nfree + np.arange(nfixed), np.arange(nfree)]).astype(int)      # path position -> pose index of the graph
    Rs, ts = [None] * npath, [None] * npath
    for t in range(npath):
        C = np.array([STEP * t, rng.normal(0, 0.05), rng.normal(0, 0.05)])
        R = _rot(rng.normal(0, 0.02, 3))                                                    # world -> camera: looking along +z
        Rs[index[t]], ts[index[t]] = R, -R @ C
    stereo_kf = {"mono": np.zeros(npath, bool), "stereo": np.ones(npath, bool), "mixed": rng.random(npath) < 0.6}[mode]
    e_point, e_cam, e_obs, e_info, pts = [], [], [], [], []

    def shift():
        a = rng.uniform(0, 2 * np.pi)
        return rng.uniform(40, 80) * np.array([np.cos(a), np.sin(a)])

    def observe(n, k, Xw):
        c = Rs[k] @ Xw + ts[k]
        u = FX * c[0] / c[2] + CX + rng.normal(0, noise_px)
        v = FY * c[1] / c[2] + CY + rng.normal(0, noise_px)
        if all_outlier_keyframe is not None and k == all_outlier_keyframe:
            s = shift()
            u += s[0]; v += s[1]
        lvl = int(rng.integers(0, 4))
        is_stereo = stereo_kf[k] and (mode == "stereo" or rng.random() < 0.8)
        ur = u - BF / c[2] + rng.normal(0, noise_px) if is_stereo else -1.0
        e_point.append(n); e_cam.append(k); e_obs.append((u, v, ur)); e_info.append(1.0 / 1.2 ** (2 * lvl))

    def cloud(t):
        return np.array([STEP * t + rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4.5, 8)])

    for t0 in range(npath):
        for _ in range(points_per_kf):
            n = len(pts)
            pts.append(cloud(t0))
            window = np.arange(max(t0 - w, 0), min(t0 + w, npath - 1) + 1)
            m = int(rng.integers(min(3, len(window)), min(8, len(window)) + 1))
            seen = rng.choice(window, m, replace=False)
            if not (seen >= nfixed).any():
                seen[0] = int(rng.integers(nfixed, min(nfixed + w, npath - 1) + 1))
                seen = np.unique(seen)
            for t in rng.permutation(seen):                                                 # the observations map's order is not the path's
                observe(n, int(index[t]), pts[n])
    for (e_lo, e_hi), (l_lo, l_hi), count in loops:
        for _ in range(count):
            n = len(pts)
            pts.append(cloud(nfixed + (e_lo + e_hi) / 2))
            for k in rng.permutation(np.concatenate([np.arange(e_lo, e_hi + 1), np.arange(l_lo, l_hi + 1)])):
                observe(n, int(k), pts[n])
    for _ in range(lonely_points):
        pts.append(np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 6.0]))
    poses = np.zeros((npath, 16), np.float32)
    for k in range(npath):
        R, t = Rs[k], ts[k]
        if k < nfree and not (kf0_fixed and k == 0):
            R = _rot(rng.normal(0, pose_err[0], 3)) @ R
            t = t + rng.normal(0, pose_err[1], 3)
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
        poses[k] = T.reshape(16)
    P = np.array(pts) + rng.normal(0, point_err, (len(pts), 3))
    fixed = np.zeros(nfree, np.uint8)
    if kf0_fixed:
        fixed[0] = 1
    e_cam = np.array(e_cam)
    if permute:
        perm = rng.permutation(nfree)                                                       # keyframe k is listed at perm[k]
        listed = np.concatenate([perm, np.arange(nfree, npath)])
        e_cam = listed[e_cam]
        poses2, fixed2 = poses.copy(), fixed.copy()
        poses2[listed] = poses; fixed2[perm] = fixed
        poses, fixed = poses2, fixed2
    ne = len(e_point)
    K = np.tile(np.array([FX, FY, CX, CY, BF], np.float32), (ne, 1))
    g = bundle.make_graph(poses, nfree, P, np.array(e_point), e_cam, np.array(e_obs, np.float64).reshape(-1, 3), np.array(e_info), K,
                          fixed if (kf0_fixed or permute) else None)
    g["truth"] = np.array(pts)                                                              # the planted points (noise-free scenes return to them)
    return g


def _local():
    return bundle.local_options()


def _global(robust, iterations=10):
    return lambda: bundle.global_options(iterations, robust)


# Keyframe 0 is fixed in the global forms, so the system is 6 (nfree - 1) wide there; the tile is 64 rows.
#   e12          n = 66: two row tiles, the last with two rows; a block straddles the tile edge
#   e33_band     n = 192: exactly three tiles, w = 4
#   e65_loop     n = 384: six full tiles; loop points between keyframes 1 - 3 and 60 - 64 (an arrow)
#   e130_robust  Huber; a loop between keyframes 20 - 22 and 70 - 72 only: first[] is not monotone
#   e70_drop     the local form; keyframe 35, in the middle, leaves the second round's system: its rows shift by 6
#   e65_shuffled e65_loop with the keyframes permuted
#   e520         one past the old limit, last tile partial
#   e1024, e4096 consistency checks only; e4096 is the capacity edge and runs optimize(3)
SPECS = [
    ("e12", dict(nfree=12, seed=501, w=3), _global(False)),
    ("e33_band", dict(nfree=33, seed=502, w=4), _global(False)),
    ("e65_loop", dict(nfree=65, seed=503, w=4, loops=(((1, 3), (60, 64), 4),)), _global(False)),
    ("e130_robust", dict(nfree=130, seed=504, w=4, loops=(((20, 22), (70, 72), 4),), lonely_points=2), _global(True)),
    ("e70_drop", dict(nfree=70, nfixed=1, seed=505, w=4, kf0_fixed=False, all_outlier_keyframe=35), _local),
    ("e65_shuffled", dict(nfree=65, seed=503, w=4, loops=(((1, 3), (60, 64), 4),), permute=True), _global(False)),
    ("e520", dict(nfree=520, seed=506, w=4), _global(False)),
    ("e1024", dict(nfree=1024, seed=507, w=6, loops=(((2, 5), (1000, 1004), 6),)), _global(False)),
    ("e4096", dict(nfree=4096, seed=508, w=8, loops=(((2, 5), (4080, 4084), 6),)), _global(False, 3)),
]
MEASURED = [s[0] for s in SPECS[:4]]            # "the new scenes up to e130": the scenes of the sensitivity file
EQUAL = MEASURED + ["e70_drop"]                 # the scenes orbm_global_bundle_adjustment takes too
_CACHE = {}


def scene(name, **override):
    """(name, graph, options), built once per process: do not write to the graph.  override: make() arguments that replace the
    scene's own (not cached)."""
    _, kw, opt = next(s for s in SPECS if s[0] == name)
    if override:
        return name, make(**dict(kw, **override)), opt()
    if name not in _CACHE:
        _CACHE[name] = (name, make(**kw), opt())
    return _CACHE[name]


def scenes(names):
    return [scene(n) for n in names]


def wide_graph():
    """A 2,048-keyframe band with the keyframes shuffled: the system has 192 row tiles, and nearly every one reaches back to the first
    columns, so the envelope is close to the full triangle of 18,528 tiles -- beyond the solver's 8,192 (tests/test_cpu_ba_env.py
    checks the count).  Two points per keyframe keep it small."""
    if "wide" not in _CACHE:
        _CACHE["wide"] = make(nfree=2048, seed=509, w=4, points_per_kf=2, permute=True)
    return _CACHE["wide"]


def numpy_envelope(blk_i1, blk_i2, ridx, T):
    """first[] of the reduced system from the listed blocks and the rows ridx[nfree] (-1: not a vertex): block (i1 <= i2) covers rows
    6 r2 .. 6 r2 + 5 from column 6 r1"""
    nact = int((ridx >= 0).sum())
    nt = (6 * nact + T - 1) // T
    first = np.arange(nt)
    for i1, i2 in zip(blk_i1, blk_i2):
        r1, r2 = ridx[i1], ridx[i2]
        if r1 < 0 or r2 < 0:
            continue
        for R in range(6 * r2 // T, (6 * r2 + 5) // T + 1):
            first[R] = min(first[R], 6 * r1 // T)
    return first.astype(np.int32)


def load_520():
    """the restatement's result on e520 in the dict form of ba_oracle.run, the hash of the inputs it was made from, and its sensitivity
    under the first 4 ulp patterns (d: poses and points, each: the entry-by-entry measures)"""
    z = np.load(GOLDEN_520)
    r = {k: z[k] for k in KEYS_520}
    r.update(iterations=z["iterations"].tolist(), trials=z["trials"].tolist(), results=z["results"].tolist(), stopped=int(z["stopped"]),
             rounds=int(z["rounds"]), ntrials=int(z["ntrials"]))
    return r, str(z["input_sha256"]), float(z["d"]), json.loads(str(z["each"]))


def write_golden():
    D, rows = ba_compare.measure_sensitivity(scenes(MEASURED))
    each = dict(ba_compare.D_EACH)
    json.dump({"note": "tests/ba_env_scenes.py write_golden(): ba_compare.measure_sensitivity on the scenes of ba_env_scenes.MEASURED -- the "
                       "restatement tests/ba_oracle.c under its +-1 ulp switch, 16 seeds per scene; the fields of ba_sensitivity.json with "
                       "D_env in D_cpu's place",
               "D_env": D, "D_each": each, "ulp_seeds": ba_compare.ULP_SEEDS, "scenes": [r["name"] for r in rows],
               "d": {r["name"]: r["d"] for r in rows}}, open(GOLDEN, "w"), indent=1)
    _, g, opt = scene("e520")
    r = ba_oracle.run(g, opt)
    d, e520 = 0.0, {}
    for seed in ba_compare.ULP_SEEDS[:4]:
        o = ba_oracle.run(g, opt, ulp_seed=seed)
        assert ba_compare.ints(o) == ba_compare.ints(r), "e520 moves an integer under an ulp pattern: choose another seed"
        d = max(d, ba_compare.rel(o["poses_d"], r["poses_d"]), ba_compare.rel(o["points_d"], r["points_d"]))
        for k, v in ba_compare.diffs_each(o, r).items():
            e520[k] = max(e520.get(k, 0.0), v)
    np.savez_compressed(GOLDEN_520, **{k: r[k] for k in KEYS_520}, iterations=np.array(r["iterations"], np.int32),
                        trials=np.array(r["trials"], np.int32), results=np.array(r["results"], np.int32), stopped=np.int32(r["stopped"]),
                        rounds=np.int32(r["rounds"]), ntrials=np.int32(r["ntrials"]), input_sha256=np.array(ba_large_scenes.input_hash(g)),
                        d=np.float64(d), each=np.array(json.dumps(e520)))
    return D, each, rows, r, d, e520


if __name__ == "__main__":
    D, each, rows, r520, d520, e520 = write_golden()
    print("D_env %.3e" % D, "D_each", each)
    for r in rows:
        log = r["base"]["trial_log"]
        print("%-14s d %.3e moved %d near %d small_rho %d trials %s accepted %d min|rho| %.3g" %
              (r["name"], r["d"], r["moved"], r["near"], r["small_rho"], r["base"]["trials"], int(log["accepted"].sum()), np.abs(log["rho"]).min()))
    log = r520["trial_log"]
    print("e520 trials", r520["trials"], "accepted", int(log["accepted"].sum()), "min|rho| %.3g" % np.abs(log["rho"]).min(), "d %.3e" % d520, e520)
