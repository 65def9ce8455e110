"""Seeded pose graphs for orbm_essential_graph (test infrastructure: never part of the product): a keyframe trajectory that drifts
and closes a loop, flattened the way integration/Optimizer_essential_graph_hip.cc flattens the reference's walk (src/Optimizer.cc
:1193-1367) -- the LoopConnections edges first, then per keyframe its spanning-tree edge, its old loop edges and its covisibility
edges.  The smallest shapes at which each thing can go wrong:
  two_v0fixed / two_v1fixed   2 vertices, 1 edge, n = 7: either side of a binary edge fixed
  ring9     10 vertices, 9 in the system, n = 63: one tile of the solver
  ring10    11 vertices, n = 70: the last block straddles the first tile boundary (64)
  tree40    41 keyframes, one of them without an edge: 40 vertices in the graph, 39 in the system, n = 273, 5 tiles: a spanning tree + covisibility edges, two old loop edges, a
            LoopConnections set, CorrectedSim3 / NonCorrectedSim3 entries with scales != 1, the fixed vertex in the middle of the list,
            one free vertex without an edge, one pair joined by two edges in opposite orientations
  tree70    70 vertices, n = 483: the largest scene compared with the restatement
each with the scale fixed and free ("_fix" / "_free").  ITER1[name]: the iteration count of form 1 (the scene passes the selection
rule of tests/essential_graph_compare.py with it); form 2 is the reference's 20.  The table scales put sigma = log(s) of an error on
both sides of Sim3::log's 1e-5 branch and the drift puts the rotation angles on both sides of d > 1 - 1e-5 (theta = 4.47e-3)."""
import functools

import numpy as np

from orb_slam2_e_amd import essential_graph as EG


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def se3(R, t):
    T = np.eye(4)
    T[:3, :3] = R; T[:3, 3] = t
    return T


def quat(R):
    """unit quaternion x y z w of a rotation matrix (w >= 0)"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[i] = s / 4; q[j] = (R[j, i] + R[i, j]) / s; q[k] = (R[k, i] + R[i, k]) / s; q[3] = (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def sim3_row(T, s):
    """[q xyzw, t, s] of the Sim3 whose matrix is [s R | t] with [R | t / s] = T ... given T = [R | t] and s: (R, t, s)"""
    return np.concatenate([quat(T[:3, :3]), T[:3, 3], [s]])


def sim3_mat(row):
    """the 4 x 4 matrix [s R | t; 0 1] of a table row"""
    x, y, z, w = row[:4] / np.linalg.norm(row[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = row[7] * R; M[:3, 3] = row[4:7]
    return M


def mat_row(M):
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    return np.concatenate([quat(M[:3, :3] / s), M[:3, 3], [s]])


def trajectory(nv, loop_at, rng, radius=4.0):
    """planted Tcw of nv keyframes: `loop_at` keyframes lead up to a circle of nv - loop_at, whose last keyframe comes back beside
    keyframe loop_at"""
    T = []
    nring = nv - loop_at
    for k in range(nv):
        if k < loop_at:
            c = np.array([radius + 0.6 * (loop_at - k), 0.0, 0.1 * (loop_at - k)]); ang = 0.0
        else:
            ang = 2 * np.pi * (k - loop_at) / (nring + 0.3)
            c = np.array([radius * np.cos(ang), radius * np.sin(ang), 0.05 * np.sin(3 * ang)])
        R = rodrigues([0.02 * np.sin(k), 0.03 * np.cos(2 * k), ang]).T
        T.append(se3(R, -R @ c))
    return T


def build(nv, loop_at, seed, fix_scale, tree=False, isolated=None, old_loops=(), drift_rot=2e-3, drift_t=2e-2, corr_scale=1.03,
          two_vertex=None):
    rng = np.random.default_rng(seed)
    true = trajectory(nv, loop_at, rng)
    # the drifting chain: a keyframe's pose from its predecessor's through the planted relative motion and a small error
    D = [true[0]]
    for k in range(1, nv):
        rel = true[k] @ np.linalg.inv(true[k - 1])
        big = (k % 3 == 0)                                   # every third step turns by more than 4.47e-3, the others by less
        noise = se3(rodrigues(rng.standard_normal(3) * (drift_rot * (4 if big else 0.5))), rng.standard_normal(3) * drift_t)
        D.append(noise @ rel @ D[k - 1])
    poses = np.stack([d.astype(np.float32) for d in D]).reshape(nv, 16)
    D = [p.reshape(4, 4).astype(np.float64) for p in poses]  # what the call sees
    cur, L = nv - 1, loop_at
    fixed = np.zeros(nv, np.uint8); fixed[L] = 1
    corrected = np.full(nv, -1, np.int32); noncorrected = np.full(nv, -1, np.int32)
    ctab, ntab = [], []
    s_c = 1.0 if fix_scale else corr_scale
    # the current keyframe's corrected Sim3: where the loop keyframe's (drifted) pose and the planted relative motion put it
    S_cur = true[cur] @ np.linalg.inv(true[L]) @ D[L]
    S_cur = np.vstack([np.hstack([s_c * S_cur[:3, :3], s_c * S_cur[:3, 3:4]]), [[0, 0, 0, 1]]])
    ncorr = 1 if two_vertex else min(3, cur - L)
    for a, k in enumerate(range(cur, cur - ncorr, -1)):      # CorrectLoop: g2oCorrectedSiw = g2oSic * mg2oScw
        M = D[k] @ np.linalg.inv(D[cur]) @ S_cur
        corrected[k] = len(ctab); ctab.append(mat_row(M))
        # (the planted table scales of the non-corrected entries: sigma = log(s) on both sides of 1e-5)
        s_n = 1.0 if fix_scale else (1.0, 1.0 + 5e-6, 1.0 + 2e-5)[a]
        noncorrected[k] = len(ntab); ntab.append(sim3_row(D[k], s_n))
    e0, e1, kind = [], [], []
    if two_vertex:
        e0, e1, kind = ([cur], [L], [1]) if two_vertex == "v0fixed" else ([L], [cur], [1])   # the fixed vertex is the edge's vertex 1 / 0
    else:
        inserted = set()
        for a, b in ((cur, L), (cur - 1, cur), (cur - 1, L)):           # the LoopConnections loop (:1236-1264)
            e0.append(a); e1.append(b); kind.append(0); inserted.add((min(a, b), max(a, b)))
        parent = {}
        for i in range(nv):
            if i == isolated:
                continue
            cand = [p for p in ((i - 1, i - 2, i - 3) if not (tree and i % 5 == 2) else (i - 2, i - 1, i - 3)) if p >= 0 and p != isolated]
            par = cand[0] if cand else None
            parent[i] = par
            if par is not None:                                          # spanning tree
                e0.append(i); e1.append(par); kind.append(1)
            loops = [b for a, b in old_loops if a == i]
            for b in loops:                                              # old loop edges (pLKF->mnId < pKF->mnId)
                e0.append(i); e1.append(b); kind.append(1)
            for d in ((2, 3, 4) if tree else (2,)):                     # covisibility, best first
                n = i - d
                if n < 0 or n == isolated or n == par or n in loops or parent.get(n) == i:
                    continue
                if (n, i) in inserted:
                    continue
                e0.append(i); e1.append(n); kind.append(1)
    # map points: a few per keyframe in front of it (planted), given in the drifted frame of their reference
    pts, ref = [], []
    for v in range(nv):
        for _ in range(3):
            Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])
            Dv = D[v]
            pts.append(Dv[:3, :3].T @ (Xc - Dv[:3, 3])); ref.append(v)
    if two_vertex == "v1fixed":                                          # the same graph with the vertices listed the other way round
        perm = np.array([1, 0])
        poses = poses[perm]; fixed = fixed[perm]; corrected = corrected[perm]; noncorrected = noncorrected[perm]
        e0 = [int(perm[a]) for a in e0]; e1 = [int(perm[a]) for a in e1]; ref = [int(perm[a]) for a in ref]
    return EG.make_graph(poses, fixed, e0, e1, kind, fix_scale, corrected, np.array(ctab), noncorrected, np.array(ntab), np.array(pts), ref)


# name -> (arguments of build without fix_scale, seeds for (fix, free)).  The drift is large enough that several Gauss-Newton-like
# steps are needed before the rounding floor (lambda starts at 1e-16); a graph of ONE edge is solved by its first step whatever the start
_FAR = dict(drift_rot=4e-2, drift_t=4e-1)
SPECS = {
    "two_v0fixed": (dict(nv=2, loop_at=0, two_vertex="v0fixed", **_FAR), (11, 12)),
    "two_v1fixed": (dict(nv=2, loop_at=0, two_vertex="v1fixed", **_FAR), (13, 14)),
    "ring9": (dict(nv=10, loop_at=0, **_FAR), (21, 22)),
    "ring10": (dict(nv=11, loop_at=0, **_FAR), (23, 24)),
    "tree40": (dict(nv=41, loop_at=17, tree=True, isolated=5, old_loops=((30, 19), (33, 21)), **_FAR), (31, 41)),
    "tree70": (dict(nv=70, loop_at=8, tree=True, old_loops=((50, 20),), drift_rot=1e-2, drift_t=1e-1), (41, 42)),
}
NAMES = [f"{n}_{s}" for n in SPECS for s in ("fix", "free")]
# form 1: the iterations with which the scene passes the selection rule (tests/test_cpu_essential_graph.py holds every scene to it)
ITER1 = {name: 5 for name in NAMES}
ITER1.update(two_v0fixed_fix=1, two_v0fixed_free=1, two_v1fixed_fix=1, two_v1fixed_free=1, tree70_free=4)
ITER2 = 20


@functools.lru_cache(maxsize=None)
def scene(name):
    base, form = name.rsplit("_", 1)
    kw, seeds = SPECS[base]
    fix = form == "fix"
    g = build(seed=seeds[0 if fix else 1], fix_scale=fix, **kw)
    for a in g.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g


def scenes(names=None):
    return [(n, scene(n)) for n in (names if names is not None else NAMES)]


def chain(nact, seed=7, edges_per_vertex=10, fix_scale=True):
    """A larger graph for the limit and the timings: nact + 1 keyframes (keyframe 0 fixed), a drifting circle closed by a loop, about
    `edges_per_vertex` edges per keyframe (the spanning tree and the covisibility edges to the nearest predecessors)."""
    nv = nact + 1
    rng = np.random.default_rng(seed)
    true = trajectory(nv, 0, rng, radius=0.08 * nv)
    D = [true[0]]
    for k in range(1, nv):
        rel = true[k] @ np.linalg.inv(true[k - 1])
        D.append(se3(rodrigues(rng.standard_normal(3) * 5e-4), rng.standard_normal(3) * 2e-3) @ rel @ D[k - 1])
    poses = np.stack([d.astype(np.float32) for d in D]).reshape(nv, 16)
    Dc = poses[-1].reshape(4, 4).astype(np.float64)
    fixed = np.zeros(nv, np.uint8); fixed[0] = 1
    corrected = np.full(nv, -1, np.int32); noncorrected = np.full(nv, -1, np.int32)
    S_cur = true[-1] @ np.linalg.inv(true[0]) @ poses[0].reshape(4, 4).astype(np.float64)
    corrected[-1] = 0; noncorrected[-1] = 0
    e0, e1, kind = [nv - 1], [0], [0]
    for i in range(1, nv):
        for d in range(1, edges_per_vertex + 1):
            if i - d >= 0 and not (i == nv - 1 and i - d == 0):
                e0.append(i); e1.append(i - d); kind.append(1)
    pts = rng.uniform(-1, 1, (4 * nv, 3)); ref = rng.integers(0, nv, 4 * nv)
    return EG.make_graph(poses, fixed, e0, e1, kind, fix_scale, corrected, np.array([mat_row(S_cur)]), noncorrected, np.array([sim3_row(Dc, 1.0)]),
                         pts, ref)


def planted_ring(nv=10, seed=5, fix_scale=True):
    """A ring whose measurements are ALL consistent with one planted configuration: every keyframe has a NonCorrectedSim3 entry, the
    planted pose, and every edge is of kind 1; the poses the optimisation starts from drift away from it (the fixed keyframe 0 starts
    where it is planted).  Returns (graph, planted [nv][8])."""
    rng = np.random.default_rng(seed)
    true = trajectory(nv, 0, rng)
    true[0] = true[0].astype(np.float32).astype(np.float64)
    D = [true[0]]
    for k in range(1, nv):
        rel = true[k] @ np.linalg.inv(true[k - 1])
        D.append(se3(rodrigues(rng.standard_normal(3) * 2e-2), rng.standard_normal(3) * 1e-1) @ rel @ D[k - 1])
    planted = np.stack([sim3_row(T, 1.0) for T in true])
    fixed = np.zeros(nv, np.uint8); fixed[0] = 1
    e0, e1 = [nv - 1], [0]
    for i in range(1, nv):
        e0.append(i); e1.append(i - 1)
        if i >= 2:
            e0.append(i); e1.append(i - 2)
    g = EG.make_graph(np.stack([d.astype(np.float32) for d in D]), fixed, e0, e1, np.ones(len(e0), np.uint8), fix_scale,
                      noncorrected=np.arange(nv), noncorrected_sim3=planted)
    return g, planted
