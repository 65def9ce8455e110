"""An independent float64 check that a Sim3 is the optimum of OptimizeSim3's second round (test infrastructure), as
tests/pose_optimum.py is for PoseOptimization.

Written from the g2o edge definitions alone (types_seven_dof_expmap.h: EdgeSim3ProjectXYZ e12 = obs1 - K1 proj(S X2),
EdgeInverseSim3ProjectXYZ e21 = obs2 - K2 proj(S^-1 X1), information = invSigma2 * I, the Huber kernel of width sqrt(th2)) in plain
numpy, with ANALYTIC Jacobians of the left-multiplicative update Sim3(u) * S, u = (omega, upsilon, sigma):
    y = S X2 = s R X2 + t:          dy = [-[y]x | I | y] u
    z = S^-1 X1 = R^T (X1 - t) / s: dz = (1 / s) R^T [[X1]x | -I | -X1] u
It shares no Jacobian, exp map or linear solver with tests/sim3_opt_oracle.c.  Both rounds keep the Huber kernel, so the cost is
sum rho(chi2) over the kept edges; one Gauss-Newton (IRLS) step from the result must be small and buy almost nothing."""
import numpy as np
from scipy.linalg import expm

from pose_optimum import GAIN_TOL, STEP_TOL, _hat, quat_matrix   # noqa: F401  (the bounds tests/test_gpu_pose_edges.py uses)

MIN_PAIRS = 10


def generator(u):
    """the 4 x 4 generator of u = (omega, upsilon, sigma): expm of it is the similarity [[e^sigma R, t], [0, 1]]"""
    G = np.zeros((4, 4))
    G[:3, :3] = _hat(u[:3]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    return G


def sim3_matrix(q, t, s):
    """[[s R, t], [0, 1]] with R the rotation of q = (x, y, z, w) normalised"""
    T = np.eye(4)
    T[:3, :3] = s * quat_matrix(q)
    T[:3, 3] = np.asarray(t, np.float64)
    return T


def exp_sim3(u):
    return expm(generator(np.asarray(u, np.float64)))


class Pairs:
    """the kept pairs of a problem dict (tests/sim3_opt_scenes.py): camera-frame points in float64 from the float inputs"""

    def __init__(self, p, inv_sigma2, kept):
        k = np.flatnonzero(np.asarray(kept))
        f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
        T1, T2 = f64(p["Tcw1"]).reshape(4, 4), f64(p["Tcw2"]).reshape(4, 4)
        self.X1 = f64(p["X1w"])[k] @ T1[:3, :3].T + T1[:3, 3]
        self.X2 = f64(p["X2w"])[k] @ T2[:3, :3].T + T2[:3, 3]
        self.obs1, self.obs2 = f64(p["obs1"])[k], f64(p["obs2"])[k]
        sg = f64(inv_sigma2)
        self.w1, self.w2 = sg[np.asarray(p["octave1"])[k]], sg[np.asarray(p["octave2"])[k]]
        self.cam1, self.cam2 = f64(p["cam1"]), f64(p["cam2"])
        self.delta = float(np.sqrt(np.float32(p["th2"])))

    @staticmethod
    def _proj(Y, cam):
        return np.stack([cam[0] * Y[:, 0] / Y[:, 2] + cam[2], cam[1] * Y[:, 1] / Y[:, 2] + cam[3]], 1)

    @staticmethod
    def _dproj(Y, cam):
        """[m, 2, 3] derivative of the projection"""
        J = np.zeros((len(Y), 2, 3))
        iz = 1.0 / Y[:, 2]
        J[:, 0, 0] = cam[0] * iz; J[:, 0, 2] = -cam[0] * Y[:, 0] * iz * iz
        J[:, 1, 1] = cam[1] * iz; J[:, 1, 2] = -cam[1] * Y[:, 1] * iz * iz
        return J

    def residuals(self, T):
        """(e [2m, 2], info [2m]): e12 of every pair, then e21"""
        sR, t = T[:3, :3], T[:3, 3]
        Y = self.X2 @ sR.T + t
        Z = (self.X1 - t) @ np.linalg.inv(sR).T
        return np.concatenate([self.obs1 - self._proj(Y, self.cam1), self.obs2 - self._proj(Z, self.cam2)]), np.concatenate([self.w1, self.w2])

    def jacobians(self, T):
        """[2m, 2, 7] analytic d e / d u at u = 0"""
        sR, t = T[:3, :3], T[:3, 3]
        s = np.cbrt(np.linalg.det(sR))
        R = sR / s
        Y = self.X2 @ sR.T + t
        Z = (self.X1 - t) @ np.linalg.inv(sR).T
        m = len(Y)
        dY = np.zeros((m, 3, 7)); dZ = np.zeros((m, 3, 7))
        for i in range(m):
            dY[i, :, :3] = -_hat(Y[i]); dY[i, :, 3:6] = np.eye(3); dY[i, :, 6] = Y[i]
            B = np.zeros((3, 7))
            B[:, :3] = _hat(self.X1[i]); B[:, 3:6] = -np.eye(3); B[:, 6] = -self.X1[i]
            dZ[i] = R.T @ B / s
        return np.concatenate([-np.einsum("mij,mjk->mik", self._dproj(Y, self.cam1), dY), -np.einsum("mij,mjk->mik", self._dproj(Z, self.cam2), dZ)])

    def huber(self, chi2):
        """(rho, weight) of RobustKernelHuber with delta"""
        d = self.delta
        big = chi2 > d * d
        sq = np.sqrt(np.where(big, chi2, 1.0))
        return np.where(big, 2 * sq * d - d * d, chi2), np.where(big, d / sq, 1.0)

    def cost(self, T):
        e, w = self.residuals(T)
        return float(np.sum(self.huber(w * np.sum(e * e, 1))[0]))


def gauss_newton_check(p, inv_sigma2, kept, q, t, s):
    """One float64 Gauss-Newton (IRLS) step on the Huber cost of the kept pairs from the Sim3 (q, t, s).  Returns (max |step|,
    relative gain of the cost, cost)."""
    assert int(np.sum(kept)) >= MIN_PAIRS
    E = Pairs(p, inv_sigma2, kept)
    T = sim3_matrix(q, t, s)
    e, w = E.residuals(T)
    J = E.jacobians(T)
    rho, hw = E.huber(w * np.sum(e * e, 1))
    W = (w * hw)[:, None, None]
    H = np.einsum("mij,mik->jk", J, W * J)
    g = np.einsum("mij,mi->j", J, (w * hw)[:, None] * e)
    if p["fix_scale"]:
        H, g = H[:6, :6], g[:6]
    step = np.linalg.solve(H, -g)
    step = np.concatenate([step, np.zeros(7 - len(step))])
    c0 = float(rho.sum())
    c1 = E.cost(exp_sim3(step) @ T)
    return float(np.abs(step).max()), (c0 - c1) / c0, c0
