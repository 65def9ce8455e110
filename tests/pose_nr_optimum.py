"""An independent float64 check of a result of PoseOptimizationNR's bundle (test infrastructure), in the spirit of
tests/pose_optimum.py: plain numpy from the definitions alone -- pinhole projection through rotation matrices, chi2 = invSigma2 |e|^2,
the Huber kernel, central-difference Jacobians of the left-multiplicative update exp(d) * T and of the points, a dense solve of the
damped normal equations, the strain energy |a^T K a| / (Ksize / 3) on the dense K.  It shares no Jacobian, exp map, Schur
complement, 3 x 3 inverse or LDLT with the kernel or with tests/pose_nr_bundle_oracle.c.

The loop of PoseOptimizationNR does not stop at a stationary point of a cost: its linear system holds the reprojection edges
alone, the energy only gates a trial (currentChi += nsE, tempChi = chi2 + 2 nsE on an iteration's first trial, + 5 nsE on its
retries), and its rounds end on ten rejected trials.  So "one Gauss-Newton step from the result is small" has no bound there.
What does follow from the loop: the result is the state of the LAST ACCEPTED trial k (every later trial was popped), hence
  (a) the robust chi2 over the edges active in k's round plus w nsE at the result IS that trial's tempChi, and
  (b) the trial after it, k + 1, is the first trial of a new iteration FROM the result with the lambda trial k left (or, where a
      new round begins there, with computeLambdaInit's): one damped
      Gauss-Newton step from the result on the edges active in k + 1's round lands where that trial's tempChi = chi2 + 2 nsE was
      measured.
Both are reproduced here from the result alone and compared with the trial log.  The step of (b) checks the Jacobians, the Schur
step, the exp map and the hook of whatever produced the log against none of its own formulas.

TOL: the energy is a float computation (the top layer is cast to float, K a runs in float on the device and in the oracle; here
in double on the float a): 1e-5 of nsE, the bound the FEM tests hold the energies to; the central differences (h = 1e-6) are good
to 1e-9 of a Jacobian entry.  tests/test_cpu_pose_nr_bundle.py measures both figures on the restatement's results and requires
them 10 x inside TOL."""
import numpy as np

TOL = 1e-5        # |reproduced tempChi - logged tempChi| / |logged tempChi|
H = 1e-6


def quat_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp_se3(d):
    """(R, t) of the SE(3) exponential of d = (omega, upsilon)"""
    w, v = np.asarray(d[:3], np.float64), np.asarray(d[3:], np.float64)
    th = np.linalg.norm(w)
    W = _hat(w)
    if th < 1e-8:
        return np.eye(3) + W + W @ W / 2, (np.eye(3) + W / 2 + W @ W / 6) @ v
    R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    return R, V @ v


def _rotation(M):
    """the rotation nearest to a 3 x 3 matrix of floats (Converter::toSE3Quat normalises the quaternion)"""
    u, _, vt = np.linalg.svd(np.asarray(M, np.float64))
    return u @ vt


class Problem:
    def __init__(self, g, K, u0, ids, derived=None, klarge=1e8):
        self.ept, self.ecam = g["e_point"], g["e_cam"]
        self.obs = g["e_obs"].astype(np.float64); self.info = g["e_inv_sigma2"].astype(np.float64); self.cam = g["e_cam_k"].astype(np.float64)
        kT = g["kf_Tcw"].reshape(-1, 4, 4)
        self.kfR = np.array([_rotation(T[:3, :3]) for T in kT]).reshape(-1, 3, 3); self.kft = kT[:, :3, 3].astype(np.float64)
        self.K = np.asarray(K); self.u0 = np.asarray(u0, np.float32); self.ids = np.asarray(ids)
        self.der = np.zeros((0, 4), np.int32) if derived is None else np.asarray(derived)
        self.klarge = np.float32(klarge)
        self.delta = float(np.float32(np.sqrt(5.991))); self.dsqr = float(np.float32(self.delta * self.delta))

    def errors(self, R, t, X):
        """reprojection errors [ne, 2] with the frame at (R, t) and the points X"""
        Re = np.where((self.ecam < 0)[:, None, None], R[None], self.kfR[np.maximum(self.ecam, 0)] if len(self.kfR) else R[None])
        te = np.where((self.ecam < 0)[:, None], t[None], self.kft[np.maximum(self.ecam, 0)] if len(self.kft) else t[None])
        c = np.einsum("eij,ej->ei", Re, X[self.ept]) + te
        proj = np.stack([c[:, 0] / c[:, 2] * self.cam[:, 0] + self.cam[:, 2], c[:, 1] / c[:, 2] * self.cam[:, 1] + self.cam[:, 3]], 1)
        return self.obs - proj

    def robust(self, err):
        """(rho, rho') of the Huber kernel per edge"""
        e2 = self.info * (err ** 2).sum(1)
        big = e2 > self.dsqr
        s = np.sqrt(np.where(big, e2, 1.0))
        return np.where(big, 2 * s * self.delta - self.dsqr, e2), np.where(big, self.delta / s, 1.0)

    def energy(self, X):
        """nsE at the point estimates X: GetPointCoordinates' cast, Set_uf's derived nodes, a = uf - u0, the Dirichlet entries"""
        n = len(self.u0)
        ntop = n // 6
        top = np.zeros((ntop, 3), np.float32)
        top[:len(X)] = X.astype(np.float32)
        for d, (c, i0, i1, i2) in enumerate(self.der):
            top[len(X) + d] = (top[i0] + top[i1]) / np.float32(2) if c == 2 else (top[i0] + top[i1] + top[i2]) / np.float32(3)
        uf = self.u0.copy()
        uf[:3 * ntop] = top.ravel()
        a = uf - self.u0
        for i in self.ids:
            a[3 * (i - 1):3 * (i - 1) + 3] = np.float32(1) / self.klarge
        a = a.astype(np.float64)
        nz = np.flatnonzero(a)
        f = self.K[:, nz].astype(np.float64) @ a[nz]
        return abs(float(a @ f)) / (n // 3)

    def cost(self, R, t, X, active, w):
        return float(self.robust(self.errors(R, t, X))[0][active].sum()) + w * self.energy(X)

    def damped_step(self, R, t, X, active, lam):
        """(R', t', X') one Levenberg step away: (J^T W J + lam I) x = -J^T W e over the active edges, W = rho' invSigma2, numeric J"""
        e0 = self.errors(R, t, X)
        wgt = (self.robust(e0)[1] * self.info)[:, None]
        pts = np.unique(self.ept[active])
        col = -np.ones(len(X), np.int64); col[pts] = 6 + 3 * np.arange(len(pts))
        nv = 6 + 3 * len(pts)
        Jp = np.zeros((len(e0), 2, 6)); Jx = np.zeros((len(e0), 2, 3))
        for j in range(6):
            d = np.zeros(6); d[j] = H
            Rp, tp = exp_se3(d); Rm, tm = exp_se3(-d)
            Jp[:, :, j] = (self.errors(Rp @ R, Rp @ t + tp, X) - self.errors(Rm @ R, Rm @ t + tm, X)) / (2 * H)
        for j in range(3):
            d = np.zeros(3); d[j] = H
            Jx[:, :, j] = (self.errors(R, t, X + d) - self.errors(R, t, X - d)) / (2 * H)
        A = np.zeros((nv, nv)); b = np.zeros(nv)
        act = np.flatnonzero(active)
        w, Ja, Jb, ea, c = wgt[act, 0], Jp[act], Jx[act], e0[act], col[self.ept[act]]
        A[:6, :6] = np.einsum("eki,e,ekj->ij", Ja, w, Ja); b[:6] = -np.einsum("eki,e,ek->i", Ja, w, ea)
        Hpl = np.einsum("eki,e,ekj->eij", Ja, w, Jb); Hll = np.einsum("eki,e,ekj->eij", Jb, w, Jb); bl = -np.einsum("eki,e,ek->ei", Jb, w, ea)
        for j in range(3):
            np.add.at(b, c + j, bl[:, j])
            for i in range(3):
                np.add.at(A, (c + i, c + j), Hll[:, i, j])
            for i in range(6):
                np.add.at(A, (np.full(len(c), i), c + j), Hpl[:, i, j]); np.add.at(A, (c + j, np.full(len(c), i)), Hpl[:, i, j])
        if lam is None:                                     # the first iteration of a round: computeLambdaInit, tau = 1e-5
            lam = 1e-5 * np.abs(np.diag(A)).max()
        x = np.linalg.solve(A + lam * np.eye(nv), b)
        Ru, tu = exp_se3(x[:6])
        Xn = X.copy()
        Xn[pts] += x[6:].reshape(-1, 3)
        return Ru @ R, Ru @ t + tu, Xn, x


def check(pb, q, t, X, trials, trials_per_round, levels):
    """From a result (q, t, X in double), its trial log and the edge levels of each round: the relative differences (a), (b) of the
    module's docstring, and the pose part of the step of (b).  (b) is None when the last accepted trial is the log's last."""
    acc = np.flatnonzero(trials["acc"] == 1)
    k = int(acc[-1])
    first = np.concatenate([[0], np.cumsum(trials_per_round)])
    rnd = lambda i: int(np.searchsorted(first, i, side="right") - 1)
    R, t, X = quat_matrix(q), np.asarray(t, np.float64), np.asarray(X, np.float64)
    w = 2.0 if trials["qmax"][k] == 0 else 5.0
    a = abs(pb.cost(R, t, X, levels[rnd(k)] == 0, w) - trials["tempChi"][k]) / abs(trials["tempChi"][k])
    if k + 1 >= len(trials):
        return a, None, None
    assert trials["qmax"][k + 1] == 0
    active = levels[rnd(k + 1)] == 0
    Rn, tn, Xn, x = pb.damped_step(R, t, X, active, float(trials["lam"][k]) if rnd(k + 1) == rnd(k) else None)
    b = abs(pb.cost(Rn, tn, Xn, active, 2.0) - trials["tempChi"][k + 1]) / abs(trials["tempChi"][k + 1])
    return a, b, float(np.abs(x[:6]).max())
