"""Float64 numpy checks of a bundle-adjustment result that share no formula with the kernels or the restatement (test
infrastructure): rotation MATRICES (the code under test works in quaternions), the projection written with plain divisions in
double (no float invz), and central differences for the Jacobians.

  edge_chi2          every edge's chi2 and depth at given estimates
  erase_list         chi2 > threshold or depth <= 0 at the RETURNED estimates: the erase list wherever the last trial was accepted
  level0_chi2        the plain chi2 over the level-0 edges
  first_trial_chi2 / next_trial_chi2   the chi2 one damped Gauss-Newton step reaches from the input / from returned estimates with
                     the last lambda (Jacobians by central differences, a dense solve)"""
import numpy as np


def quat_to_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_matrices(g, poses_d):
    """R [npose][3][3], t [npose][3]: the free keyframes from the result's (q, t) -- a fixed or unconnected one, and every fixed
    keyframe, from the graph's 4 x 4 floats"""
    P = g["poses"].reshape(-1, 4, 4).astype(np.float64)
    R, t = P[:, :3, :3].copy(), P[:, :3, 3].copy()
    connected = np.zeros(len(P), bool); connected[g["e_cam"]] = True
    for k in range(g["nfree"]):
        if connected[k] and not (g["fixed"] is not None and g["fixed"][k]):
            R[k] = quat_to_R(poses_d[k, :4]); t[k] = poses_d[k, 4:]
    return R, t


def residuals(g, R, t, X):
    """[nedges][3] (third entry 0 for a monocular edge) and the depths"""
    cam = g["e_cam"]
    c = np.einsum("eij,ej->ei", R[cam], X[g["e_point"]]) + t[cam]
    K = g["e_cam_k"].astype(np.float64); obs = g["e_obs"].astype(np.float64)
    u = K[:, 0] * c[:, 0] / c[:, 2] + K[:, 2]
    v = K[:, 1] * c[:, 1] / c[:, 2] + K[:, 3]
    ur = u - K[:, 4] / c[:, 2]
    stereo = obs[:, 2] >= 0
    r = np.column_stack([obs[:, 0] - u, obs[:, 1] - v, np.where(stereo, obs[:, 2] - ur, 0.0)])
    return r, c[:, 2]


def edge_chi2(g, poses_d, points_d):
    R, t = pose_matrices(g, poses_d)
    r, depth = residuals(g, R, t, np.asarray(points_d, np.float64))
    return (r * r).sum(1) * g["e_inv_sigma2"].astype(np.float64), depth


def erase_list(g, opt, poses_d, points_d):
    chi2, depth = edge_chi2(g, poses_d, points_d)
    th = np.where(g["e_obs"][:, 2] < 0, opt.chi2_mono, opt.chi2_stereo)
    return ((chi2 > th) | ~(depth > 0)).astype(np.uint8), chi2, th


def level0_chi2(g, poses_d, points_d, level):
    chi2, _ = edge_chi2(g, poses_d, points_d)
    return float(chi2[np.asarray(level) == 0].sum())


def _so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K, np.eye(3) + 0.5 * K
    A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * K + B * K @ K, np.eye(3) + B * K + Cc * K @ K


def gn_step_chi2(g, R0, t0, X0, lam=None):
    """From the estimates (R0, t0, X0) of a graph without robust kernels: one damped Gauss-Newton step of the whole (poses + points)
    system solved densely with lambda (None: 1e-5 times the largest diagonal entry of J^T W J, computeLambdaInit), the update
    applied as exp(delta) * T and X + delta, and the chi2 there: what a Levenberg trial's tempChi must be.  J by central
    differences (h = 1e-6: truncation and rounding both below 1e-7 of an entry).  Returns (lambda, chi2 before, chi2 after)."""
    P = g["poses"].reshape(-1, 4, 4)
    connected = np.zeros(len(P), bool); connected[g["e_cam"]] = True
    free = [k for k in range(g["nfree"]) if connected[k] and not (g["fixed"] is not None and g["fixed"][k])]
    pts = np.unique(g["e_point"])
    w = np.repeat(g["e_inv_sigma2"].astype(np.float64), 3)

    def at(delta):
        R, t, X = R0.copy(), t0.copy(), X0.copy()
        for i, k in enumerate(free):
            d = delta[6 * i:6 * i + 6]
            dR, V = _so3(d[:3])
            R[k] = dR @ R0[k]; t[k] = dR @ t0[k] + V @ d[3:]
        X[pts] += delta[6 * len(free):].reshape(-1, 3)
        return residuals(g, R, t, X)[0].ravel()

    n = 6 * len(free) + 3 * len(pts)
    r0 = at(np.zeros(n))
    J = np.zeros((len(r0), n))
    h = 1e-6
    for j in range(n):
        d = np.zeros(n); d[j] = h
        J[:, j] = (at(d) - at(-d)) / (2 * h)
    H = J.T @ (w[:, None] * J)
    b = -J.T @ (w * r0)
    if lam is None:
        lam = 1e-5 * np.abs(np.diag(H)).max()
    delta = np.linalg.solve(H + lam * np.eye(n), b)
    r1 = at(delta)
    return lam, float((w * r0 * r0).sum()), float((w * r1 * r1).sum())


def first_trial_chi2(g):
    """gn_step_chi2 from the INPUT estimates with computeLambdaInit's lambda: the first Levenberg trial"""
    P = g["poses"].reshape(-1, 4, 4).astype(np.float64)
    return gn_step_chi2(g, P[:, :3, :3].copy(), P[:, :3, 3].copy(), g["points"].astype(np.float64))


def next_trial_chi2(g, poses_d, points_d, lam):
    """gn_step_chi2 from RETURNED estimates with the last lambda: the trial a further iteration would open with"""
    R, t = pose_matrices(g, poses_d)
    return gn_step_chi2(g, R, t, np.asarray(points_d, np.float64).copy(), lam)
