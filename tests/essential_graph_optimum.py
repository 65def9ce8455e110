"""An independent float64 model of the essential graph's cost (test infrastructure: never part of the product).  It shares no formula
with the kernel or the restatement: a Sim3 is its 4 x 4 matrix [s R | t; 0 1], products and inverses are numpy's, and the error of an
edge is the 7 coordinates of a matrix LOGARITHM of its own (inverse scaling and squaring: square roots by the Denman-Beavers
iteration, then the series of log(I + X)), read off the generator [[sigma I + [omega]x, upsilon], [0, 0]].  Where the reference's
Sim3::log is the exact logarithm the two agree; its B coefficient of the branch theta -> 0, sigma != 0 (types/sim3.h:199) is not (it
lacks the - 1), so the model is compared on graphs whose scale is fixed."""
import numpy as np

import essential_graph_scenes as S


def _sqrtm(A, iters=14):
    """batched principal square root, Denman-Beavers"""
    Y = A.copy(); Z = np.broadcast_to(np.eye(4), A.shape).copy()
    for _ in range(iters):
        Yi, Zi = np.linalg.inv(Y), np.linalg.inv(Z)
        Y, Z = 0.5 * (Y + Zi), 0.5 * (Z + Yi)
    return Y


def logm(A, roots=7, terms=14):
    """batched matrix logarithm of [B][4][4] matrices near enough to I for the principal branch"""
    A = np.asarray(A, np.float64)
    for _ in range(roots):
        A = _sqrtm(A)
    X = A - np.eye(4)
    P = X.copy(); L = X.copy()
    for n in range(2, terms + 1):
        P = P @ X
        L = L + ((-1) ** (n + 1) / n) * P
    return L * 2.0 ** roots


def expm(G, squarings=6, terms=12):
    G = np.asarray(G, np.float64) / 2.0 ** squarings
    E = np.broadcast_to(np.eye(4), G.shape).copy(); P = E.copy()
    for n in range(1, terms + 1):
        P = P @ G / n
        E = E + P
    for _ in range(squarings):
        E = E @ E
    return E


def generator(u):
    """[B][7] (omega, upsilon, sigma) -> [B][4][4]"""
    u = np.atleast_2d(np.asarray(u, np.float64))
    G = np.zeros((len(u), 4, 4))
    G[:, 0, 1] = -u[:, 2]; G[:, 0, 2] = u[:, 1]; G[:, 1, 2] = -u[:, 0]
    G[:, 1, 0] = u[:, 2]; G[:, 2, 0] = -u[:, 1]; G[:, 2, 1] = u[:, 0]
    for k in range(3):
        G[:, k, k] = u[:, 6]
    G[:, :3, 3] = u[:, 3:6]
    return G


def coordinates(L):
    """[B][4][4] generators -> [B][7]"""
    return np.stack([0.5 * (L[:, 2, 1] - L[:, 1, 2]), 0.5 * (L[:, 0, 2] - L[:, 2, 0]), 0.5 * (L[:, 1, 0] - L[:, 0, 1]), L[:, 0, 3], L[:, 1, 3],
                     L[:, 2, 3], (L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2]) / 3.0], axis=1)


def matrices(rows):
    """[n][8] (q xyzw, t, s) -> [n][4][4]"""
    return np.stack([S.sim3_mat(r) for r in np.asarray(rows, np.float64)])


def start(g):
    """(vScw [nvert][4][4], measurements [nedges][4][4]) of a graph dict, built with numpy products"""
    nv = len(g["poses"])
    P = g["poses"].reshape(nv, 4, 4).astype(np.float64)
    V = P.copy()
    ct, nt = matrices(g["corrected_sim3"]) if len(g["corrected_sim3"]) else None, matrices(g["noncorrected_sim3"]) if len(g["noncorrected_sim3"]) else None
    for v in range(nv):
        if g["corrected"][v] >= 0:
            V[v] = ct[g["corrected"][v]]
    N = V.copy()
    for v in range(nv):
        if g["noncorrected"][v] >= 0:
            N[v] = nt[g["noncorrected"][v]]
    M = []
    for i, j, k in zip(g["e_v0"], g["e_v1"], g["e_kind"]):
        Si, Sj = (V[i], V[j]) if k == 0 else (N[i], N[j])
        M.append(Sj @ np.linalg.inv(Si))
    return V, np.stack(M) if M else np.zeros((0, 4, 4))


def errors(g, M, est):
    """[nedges][7]: log(M_e S_i S_j^-1)"""
    E = M @ est[g["e_v0"]] @ np.linalg.inv(est[g["e_v1"]])
    return coordinates(logm(E))


def cost(g, M, est):
    return float((errors(g, M, est) ** 2).sum())


def gradient_norm(g, M, est, h=1e-6):
    """2-norm of the central-difference gradient of the cost over exp(h e_d) S_v of every free vertex that has an edge (with the
    scale fixed: d = 0 .. 5).  Only the edges of the perturbed vertex are evaluated again; all of them in one batch."""
    e0, e1 = g["e_v0"], g["e_v1"]
    dims = 6 if g["fix_scale"] else 7
    free = [v for v in range(len(est)) if not g["fixed"][v] and ((e0 == v) | (e1 == v)).any()]
    A, B, Ms, key = [], [], [], []
    for v in free:
        inc = np.nonzero((e0 == v) | (e1 == v))[0]
        for d in range(dims):
            for sgn in (1.0, -1.0):
                u = np.zeros(7); u[d] = sgn * h
                Pv = expm(generator(u))[0] @ est[v]
                for e in inc:
                    A.append(Pv if e0[e] == v else est[e0[e]]); B.append(Pv if e1[e] == v else est[e1[e]]); Ms.append(M[e])
                    key.append((v, d, sgn))
    E = np.stack(Ms) @ np.stack(A) @ np.linalg.inv(np.stack(B))
    c = (coordinates(logm(E)) ** 2).sum(axis=1)
    grad = {}
    for (v, d, sgn), ce in zip(key, c):
        grad[(v, d)] = grad.get((v, d), 0.0) + sgn * ce / (2 * h)
    return float(np.sqrt(sum(x * x for x in grad.values())))
