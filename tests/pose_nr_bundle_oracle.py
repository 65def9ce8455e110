"""ctypes wrapper of tests/pose_nr_bundle_oracle.c, the CPU restatement of the bundle of Optimizer::PoseOptimizationNR for the device
kernel k_pose_nr (test infrastructure: never part of the product).  The C file is compiled on first use into a per-user cache
directory (tests/c_oracle.py) and linked against the oracle's library, whose FEM hook it calls.  Also: the flat float graph both
the restatement and the device take, made from a tests/pose_nr_scene.py scene."""
import ctypes as C
import os

import numpy as np

import c_oracle
import oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "pose_nr_bundle_oracle.c")
_LIB = None

TRIAL_DTYPE = np.dtype([("sE", "<f4"), ("nsE", "<f4"), ("tempChi", "<f8"), ("currentChi", "<f8"), ("rho", "<f8"), ("lam", "<f8"),
                        ("qmax", "<i4"), ("acc", "<i4"), ("diff", "<f8")], align=True)


class SE3(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3)]


def lib():
    global _LIB
    if _LIB is None:
        so = oracle.build()
        d, name = os.path.split(so)
        flags = ("-O2", "-Wl,--no-as-needed", "-L" + d, "-l:" + name, "-Wl,-rpath," + d)
        L = C.CDLL(c_oracle.build(_SRC, [os.path.join(_HERE, "g2o_restated.h")], flags=flags))
        vp, i, d_, f = C.c_void_p, C.c_int, C.c_double, C.c_float
        graph = [i, i, i] + [vp] * 8
        L.nrb_pose_optimization_nr.argtypes = graph + [vp, i, vp, vp, i, vp, i, f, vp, i, vp, i] + [vp] * 11
        L.nrb_pose_optimization_nr.restype = i
        L.nrb_first_step.argtypes = graph + [d_] + [vp] * 6
        L.nrb_first_step.restype = i
        L.nrb_edge.argtypes = [C.POINTER(SE3)] + [vp] * 6
        L.nrb_from_cv.argtypes = [vp, C.POINTER(SE3)]
        L.nrb_oplus_pose.argtypes = [C.POINTER(SE3), vp, C.POINTER(SE3)]
        L.nrb_quat_to_matrix.argtypes = [vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def graph_from_scene(sc):
    """The flat graph of include/fem_hip.h (orbm_pose_nr_graph) from a pose_nr_scene: everything as the floats the reference holds."""
    def T(R, t):
        M = np.eye(4, dtype=np.float32)
        M[:3, :3] = np.asarray(R).reshape(3, 3); M[:3, 3] = t
        return M.reshape(16)
    nkf = len(sc["kfR"])
    return {"Tcw": np.ascontiguousarray(T(sc["R0"], sc["t0"])),
            "kf_Tcw": np.ascontiguousarray(np.array([T(sc["kfR"][k], sc["kft"][k]) for k in range(nkf)], np.float32).reshape(nkf, 16)),
            "points": np.ascontiguousarray(sc["X0"], np.float32), "e_point": np.ascontiguousarray(sc["e_pt"], np.int32),
            "e_cam": np.ascontiguousarray(sc["e_cam"], np.int32), "e_obs": np.ascontiguousarray(sc["e_obs"], np.float32),
            "e_inv_sigma2": np.ascontiguousarray(sc["e_info"], np.float32), "e_cam_k": np.ascontiguousarray(sc["e_K"], np.float32)}


def scene_from_graph(g):
    """The same values as a mini-g2o scene in double (oracle.pose_optimization_nr's input): the yardstick then sees what the
    restatement and the device see, and differs from them only in its arithmetic."""
    T = g["Tcw"].reshape(4, 4).astype(np.float64)
    kT = g["kf_Tcw"].reshape(-1, 4, 4).astype(np.float64)
    return {"R0": np.ascontiguousarray(T[:3, :3]), "t0": np.ascontiguousarray(T[:3, 3]),
            "kfR": np.ascontiguousarray(kT[:, :3, :3].reshape(-1, 9)), "kft": np.ascontiguousarray(kT[:, :3, 3]),
            "X0": np.ascontiguousarray(g["points"], np.float64), "e_pt": g["e_point"], "e_cam": g["e_cam"],
            "e_obs": np.ascontiguousarray(g["e_obs"], np.float64), "e_info": np.ascontiguousarray(g["e_inv_sigma2"], np.float64),
            "e_K": np.ascontiguousarray(g["e_cam_k"], np.float64)}


def _graph_args(g):
    return [len(g["points"]), len(g["kf_Tcw"]), len(g["e_point"])] + [_p(g[k]) for k in ("Tcw", "kf_Tcw", "points", "e_point", "e_cam", "e_obs",
                                                                                            "e_inv_sigma2", "e_cam_k")]


def pose_optimization_nr(g, K, u0, ids, derived=None, Klarge=100000000.0):
    """The restatement on the flat graph g with the oracle's FEM hook on the dense K (after ImposeDirichletEncastre_K).  Returns a dict:
    trials[TRIAL_DTYPE], results, iterations[4], trials_per_round[4], q, t, X (double), Tcw float32[4, 4], points float32[n, 3],
    outlier, ngood, class_margin[4] (the smallest |chi2 - 5.991| of each classification pass), levels[4, ne] (an edge's level while
    each round ran)."""
    L = lib()
    der = np.ascontiguousarray(derived if derived is not None else np.zeros((0, 4)), np.int32).reshape(-1, 4)
    K = np.ascontiguousarray(K, np.float32); u0 = np.ascontiguousarray(u0, np.float32); ids = np.ascontiguousarray(ids, np.int32)
    n = len(g["points"])
    assert TRIAL_DTYPE.itemsize == 56
    trials = np.zeros(400, TRIAL_DTYPE); results = np.zeros(40, np.int32); nres = C.c_int(0); rs = np.zeros(8, np.int32)
    q = np.zeros(4); t = np.zeros(3); X = np.zeros((n, 3)); Tcw = np.zeros(16, np.float32); pts = np.zeros((n, 3), np.float32)
    out = np.zeros(n, np.uint8); inl = C.c_int(0); cm = np.zeros(4); lv = np.zeros((4, len(g["e_point"])), np.int32)
    nt = L.nrb_pose_optimization_nr(*_graph_args(g), _p(K), len(K), _p(u0), _p(ids), len(ids), _p(der), len(der), Klarge, _p(trials),
                                    len(trials), _p(results), len(results), C.addressof(nres), _p(rs), _p(q), _p(t), _p(X), _p(Tcw), _p(pts),
                                    _p(out), C.addressof(inl), _p(cm), _p(lv))
    assert nt >= 0, "trial log overflow"
    return {"trials": trials[:nt].copy(), "results": results[:nres.value].copy(), "iterations": rs[:4].copy(), "trials_per_round": rs[4:].copy(),
            "q": q, "t": t, "X": X, "Tcw": Tcw.reshape(4, 4), "points": pts, "outlier": out, "ngood": inl.value, "class_margin": cm, "levels": lv}


def first_step(g, lam):
    """The linear system at the initial estimates and one damped Schur step: (ok2, Hpp[6, 6], bp[6], Hll[n, 3, 3], bl[n, 3], Hpl[n, 6, 3], x)."""
    n = len(g["points"])
    Hpp = np.zeros((6, 6)); bp = np.zeros(6); Hll = np.zeros((n, 3, 3)); bl = np.zeros((n, 3)); Hpl = np.zeros((n, 6, 3)); x = np.zeros(6 + 3 * n)
    ok = lib().nrb_first_step(*_graph_args(g), float(lam), _p(Hpp), _p(bp), _p(Hll), _p(bl), _p(Hpl), _p(x))
    return ok, Hpp, bp, Hll, bl, Hpl, x


def se3_from_cv(T):
    s = SE3()
    lib().nrb_from_cv(_p(np.ascontiguousarray(T, np.float32).reshape(16)), C.byref(s))
    return s


def oplus_pose(est, u):
    s = SE3()
    lib().nrb_oplus_pose(C.byref(est), _p(np.ascontiguousarray(u, np.float64)), C.byref(s))
    return s


def edge(T, X, obs, K):
    """(error[2], A = d error / d point [2, 3], B = d error / d pose [2, 6]) of one EdgeSE3ProjectXYZ"""
    err = np.zeros(2); A = np.zeros(6); B = np.zeros(12)
    lib().nrb_edge(C.byref(T), _p(np.ascontiguousarray(X, np.float64)), _p(np.ascontiguousarray(obs, np.float32)),
                   _p(np.ascontiguousarray(K, np.float32)), _p(err), _p(A), _p(B))
    return err, A.reshape(2, 3), B.reshape(2, 6)


def quat_to_matrix(q):
    R = np.zeros(9)
    lib().nrb_quat_to_matrix(_p(np.ascontiguousarray(q, np.float64)), _p(R))
    return R.reshape(3, 3)


def fixture_problem(name, seed, derived=None):
    """One of the closed-loop scenes of tests/test_gpu_fem.py::test_pose_optimization_nr_closed_loop on a golden surface mesh: returns
    (top, tris, graph, yardstick scene, dense K after the Dirichlet penalty, u0, ids)."""
    from pose_nr_scene import make_scene
    m = np.load(os.path.join(_HERE, "golden", f"fem_mesh_{name}.npz"))
    top, tris = m["points"], clean_triangles(m["points"], m["triangles"])
    ntop = len(top)
    nodes = oracle.fem_second_layer(top, 0.5)
    ids = np.arange(ntop, 2 * ntop, dtype=np.int32)
    K = oracle.fem_dirichlet_K(oracle.fem_assemble_dense(2, nodes, np.ascontiguousarray(np.concatenate([tris, tris + ntop], 1), np.int32)), ids)
    nv = ntop - (0 if derived is None else len(derived))
    sc = make_scene(top[:nv], seed=seed, deform=0.003, noise_px=0.5, pose_err=(0.005, 0.01))
    g = graph_from_scene(sc)
    return top, tris, g, scene_from_graph(g), K, nodes.ravel(), ids


def clean_triangles(top, tris):
    """The triangles no two corners of which coincide (what tests/test_gpu_fem.py::_clean keeps: a zero Jacobian gives a NaN K_e)."""
    p = top[tris]
    ok = ~((p[:, 0] == p[:, 1]).all(1) | (p[:, 0] == p[:, 2]).all(1) | (p[:, 1] == p[:, 2]).all(1))
    return np.ascontiguousarray(tris[ok])


def quads_from_triangles(tris):
    """Pairs of triangles that share an edge joined into quadrilaterals (a, d, b, c) -- (a, b, c) and its neighbour (b, a, d) across
    the edge a b --, greedily in triangle order; a triangle without a free neighbour is left out.  Test input only: the reference's
    tri2quad is PCL-side meshing."""
    tris = np.asarray(tris, np.int32)
    by_edge = {}
    for t, (a, b, c) in enumerate(tris):
        for u, v in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(u, v), max(u, v)), []).append(t)
    used = np.zeros(len(tris), bool)
    quads = []
    for t, (a, b, c) in enumerate(tris):
        if used[t]:
            continue
        for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
            other = [o for o in by_edge[(min(u, v), max(u, v))] if o != t and not used[o]]
            if not other:
                continue
            d = [x for x in tris[other[0]] if x != u and x != v]
            if len(d) != 1 or d[0] == w:
                continue
            quads.append([u, d[0], v, w])
            used[t] = used[other[0]] = True
            break
    return np.array(quads, np.int32).reshape(-1, 4)


def derived_nodes(nv, nder, rng):
    """vNewPointsBase for the last nder top-layer nodes, as tests/test_gpu_fem.py::test_pose_optimization_nr_fem_sequence draws them:
    mid-edge (2 bases) and barycentre (3 bases) nodes, every fifth one allowed to build on an earlier derived node"""
    der = []
    for d in range(nder):
        hi = nv + d if d % 5 == 4 else nv
        der.append([2, *rng.integers(0, hi, 2), 0] if d % 2 == 0 else [3, *rng.integers(0, hi, 3)])
        if d % 5 == 4:
            der[-1][1] = nv + d - 1                 # ... and this one does: on the derived node before it
    return np.array(der, np.int32).reshape(-1, 4)


def hex_problem(name, seed, nder):
    """A C3D8 (nElType 1) problem with derived nodes on a golden surface mesh: the first ntop - nder top nodes are the optimiser's
    points, the rest are recomputed from them by the hook.  Returns (top, quads, derived, graph, yardstick scene, K, u0, ids)."""
    from pose_nr_scene import make_scene
    m = np.load(os.path.join(_HERE, "golden", f"fem_mesh_{name}.npz"))
    top = m["points"]
    quads = quads_from_triangles(clean_triangles(top, m["triangles"]))
    ntop = len(top)
    nv = ntop - nder
    der = derived_nodes(nv, nder, np.random.default_rng(ntop))
    top = top.copy()
    for d, (c, i0, i1, i2) in enumerate(der):      # the mesh's derived nodes lie where Set_uf puts them: no strain before anything moves
        top[nv + d] = (top[i0] + top[i1]) / np.float32(2) if c == 2 else (top[i0] + top[i1] + top[i2]) / np.float32(3)
    nodes = oracle.fem_second_layer(top, 0.5)
    ids = np.arange(ntop, 2 * ntop, dtype=np.int32)
    K = oracle.fem_dirichlet_K(oracle.fem_assemble_dense(1, nodes, np.ascontiguousarray(np.concatenate([quads, quads + ntop], 1), np.int32)), ids)
    sc = make_scene(top[:nv], seed=seed, deform=0.003, noise_px=0.5, pose_err=(0.005, 0.01))
    g = graph_from_scene(sc)
    return top, quads, der, g, scene_from_graph(g), K, nodes.ravel(), ids
