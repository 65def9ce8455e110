"""An independent float64 check that a pose is the optimum of PoseOptimization's last round (test infrastructure).

Written from the g2o edge definitions alone (types_six_dof_expmap.cpp: EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
computeError with cam_project, information = invSigma2 * I, chi2 = e^T Omega e) in plain numpy: it shares no Jacobian, exp map or
linear solver with tests/pose_only_oracle.c.  Round 4 has no robust kernel and restarts from Tcw_in, so where it stopped by
Raul's criterion its estimate should sit at the minimum of the plain chi2 over the edges it had active: one Gauss-Newton step
from there, with a numeric Jacobian of the left-multiplicative SE(3) update exp(d) * T, must be small and buy almost nothing.

STEP_TOL and GAIN_TOL were calibrated on the CPU restatement (tests/test_cpu_pose_only.py checks that every calibration scene
stays 10x inside both)."""
import numpy as np

STEP_TOL = 1e-4       # max |d| of the Gauss-Newton step: radians (rotation part), metres (translation part)
GAIN_TOL = 2e-6       # (chi2(T) - chi2(exp(d) T)) / chi2(T)
MIN_EDGES = 20        # a check needs an overdetermined last round

# scenes for the device check (tests/test_gpu_pose_edges.py) and the calibration: name -> (seed, n, stereo fraction, outlier
# fraction, make_problem arguments).  On each no classification of the restatement lies near its threshold and round 4 stops
# by Raul's criterion.
SCENES = {
    "mono_60": (353, 60, 0.0, 0.1, {"noise_px": 2.0}),
    "mono_150_far": (203, 150, 0.0, 0.1, {"noise_px": 1.5, "rot_deg": 10.0, "trans_m": 0.2}),
    "mono_300": (225, 300, 0.0, 0.2, {"noise_px": 1.5}),
    "mono_1000": (209, 1000, 0.0, 0.3, {}),
    "mono_8192": (200, 8192, 0.0, 0.2, {"fill": 1.0}),
    "stereo_60": (200, 60, 1.0, 0.1, {"fill": 1.0}),
    "stereo_400_pyr6": (200, 400, 0.8, 0.15, {"nlevels": 6, "scale": 1.1}),
    "stereo_1000": (203, 1000, 1.0, 0.2, {}),
    "stereo_8192": (200, 8192, 1.0, 0.1, {"fill": 1.0}),
    "mixed_300": (202, 300, 0.5, 0.2, {}),
    "mixed_600_noisy": (200, 600, 0.3, 0.4, {"noise_px": 1.5}),
    "mixed_2000": (201, 2000, 0.4, 0.3, {}),
    "mixed_8192": (204, 8192, 0.5, 0.25, {"fill": 1.0}),
}


def quat_matrix(q):
    """Rotation matrix of the unit quaternion q = (x, y, z, w)."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp_se3(d):
    """SE(3) exponential of d = (omega, upsilon) as a 4 x 4 matrix (Rodrigues' formula and the left Jacobian V)."""
    w, v = np.asarray(d[:3], np.float64), np.asarray(d[3:], np.float64)
    th = np.linalg.norm(w)
    W = _hat(w)
    if th < 1e-8:
        R = np.eye(3) + W + W @ W / 2
        V = np.eye(3) + W / 2 + W @ W / 6
    else:
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


def pose_matrix(q, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = quat_matrix(q), np.asarray(t, np.float64)
    return T


class Edges:
    """The edges of one problem that a round had active: obs (u, v, ur), Xw, information, stereo (all float64)."""

    def __init__(self, p, active_kp):
        k = np.asarray(active_kp, np.int64)
        cam = np.asarray(p["cam"], np.float32).astype(np.float64)
        self.fx, self.fy, self.cx, self.cy, self.bf = cam
        ur = np.full(len(p["has_mp"]), -1.0, np.float32) if p["uright"] is None else np.asarray(p["uright"], np.float32)
        self.stereo = ~(ur[k] < 0)
        self.obs = np.stack([p["kp_xy"][k, 0], p["kp_xy"][k, 1], np.where(self.stereo, ur[k], 0)], 1).astype(np.float64)
        self.Xw = np.asarray(p["mp_pos"], np.float32)[k].astype(np.float64)
        self.info = np.asarray(p["inv_sigma2"], np.float32)[np.asarray(p["octave"])[k]].astype(np.float64)

    def residuals(self, T):
        """Whitened residuals sqrt(info) * e, [m, 3] (the third row 0 on monocular edges)."""
        Pc = self.Xw @ T[:3, :3].T + T[:3, 3]
        u = Pc[:, 0] / Pc[:, 2] * self.fx + self.cx
        v = Pc[:, 1] / Pc[:, 2] * self.fy + self.cy
        e = np.stack([self.obs[:, 0] - u, self.obs[:, 1] - v, np.where(self.stereo, self.obs[:, 2] - (u - self.bf / Pc[:, 2]), 0)], 1)
        return e * np.sqrt(self.info)[:, None]

    def chi2(self, T):
        return float(np.sum(self.residuals(T) ** 2))


def gauss_newton_check(p, active_kp, q, t, h=1e-6):
    """One float64 Gauss-Newton step on the plain chi2 of the edges at keypoints active_kp (at least MIN_EDGES), from the pose
    (q, t).  Returns (max |step|, relative chi2 gain, chi2)."""
    assert len(active_kp) >= MIN_EDGES
    E = Edges(p, active_kp)
    T = pose_matrix(q, t)
    r0 = E.residuals(T).ravel()
    J = np.zeros((len(r0), 6))
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        rp = E.residuals(exp_se3(d) @ T).ravel()
        d[j] = -h
        rm = E.residuals(exp_se3(d) @ T).ravel()
        J[:, j] = (rp - rm) / (2 * h)
    step = np.linalg.solve(J.T @ J, -J.T @ r0)
    c0 = float(r0 @ r0)
    c1 = E.chi2(exp_se3(step) @ T)
    return float(np.abs(step).max()), (c0 - c1) / c0, c0


def round4_active(edges):
    """Keypoint indices of the edges round 4 optimised (pose_only_oracle.run(..., edges=True)'s edge table)."""
    return edges["kp"][edges["level_r4"] == 0]
