"""Sim3Solver (src/Sim3Solver.cc) over orbm_sim3_hypotheses: the reference's interface, with every RANSAC hypothesis of one or
several candidate keyframes evaluated on the device in one call and iterate() as the reference's fold over the stored counts.

One difference to the reference: the draws of one solver are made together, at its first evaluation; in LoopClosing::ComputeSim3
they interleave with the other candidates' draws in five-iteration rounds.  Results equal the reference run whose RNG hands each
solver these triples (the reference seeds nothing here)."""
import ctypes as C
import math

import numpy as np

from ._lib import check, lib, ptr as _p


class _CSim3Problem(C.Structure):
    """orbm_sim3_problem"""
    _fields_ = [("X1w", C.c_void_p), ("X2w", C.c_void_p), ("octave1", C.c_void_p), ("octave2", C.c_void_p), ("Tcw1", C.c_void_p),
                ("Tcw2", C.c_void_p), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float), ("fx2", C.c_float),
                ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("triples", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32),
                ("fix_scale", C.c_int32)]


class _CSim3OptProblem(C.Structure):
    """orbm_sim3_opt_problem"""
    _fields_ = [("X1w", C.c_void_p), ("X2w", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p), ("octave1", C.c_void_p),
                ("octave2", C.c_void_p), ("Tcw1", C.c_void_p), ("Tcw2", C.c_void_p), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float),
                ("cy1", C.c_float), ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("R12", C.c_float * 9),
                ("t12", C.c_float * 3), ("s12", C.c_float), ("th2", C.c_float), ("fix_scale", C.c_int32), ("n", C.c_int32)]


class Sim3OptResult(C.Structure):
    """orbm_sim3_opt_result: the final g2o::Sim3 (q = x y z w), nin = the reference's return value"""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("nin", C.c_int32), ("nbad", C.c_int32),
                ("ncorrespondences", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("chi2", C.c_double)]


HYPOTHESIS_DTYPE = np.dtype([("T12", "f4", 16), ("R12", "f4", 9), ("t12", "f4", 3), ("s12", "f4"), ("ninliers", "i4")])   # orbm_sim3_hypothesis

MAX_PROBLEMS, MAX_N, MAX_H = 64, 8192, 1024


class Sim3Problem:
    """orbm_sim3_problem: the pairs the reference's constructor keeps (:64-101), flat.  cam = (fx, fy, cx, cy)."""

    def __init__(self, X1w, X2w, octave1, octave2, Tcw1, Tcw2, cam1, cam2, triples, fix_scale=False):
        f = np.ascontiguousarray
        self.X1w, self.X2w = f(X1w, np.float32).reshape(-1, 3), f(X2w, np.float32).reshape(-1, 3)
        self.octave1, self.octave2 = f(octave1, np.int32), f(octave2, np.int32)
        self.Tcw1, self.Tcw2 = f(Tcw1, np.float32).reshape(16), f(Tcw2, np.float32).reshape(16)
        self.cam1, self.cam2 = tuple(float(v) for v in cam1), tuple(float(v) for v in cam2)
        self.triples = f(triples, np.int32).reshape(-1, 3)
        self.fix_scale = bool(fix_scale)
        self.n, self.H = len(self.X1w), len(self.triples)
        if not (len(self.X2w) == len(self.octave1) == len(self.octave2) == self.n):
            raise ValueError("X1w, X2w, octave1, octave2 differ in length")

    def c(self):
        return _CSim3Problem(_p(self.X1w), _p(self.X2w), _p(self.octave1), _p(self.octave2), _p(self.Tcw1), _p(self.Tcw2), *self.cam1,
                             *self.cam2, _p(self.triples), self.n, self.H, int(self.fix_scale))


def sim3_hypotheses(problems, level_sigma2):
    """orbm_sim3_hypotheses: per problem (hyp [H] of HYPOTHESIS_DTYPE, masks [H, (n + 63) // 64] uint64)"""
    P = len(problems)
    sg = np.ascontiguousarray(level_sigma2, np.float32)
    arr = (_CSim3Problem * max(P, 1))(*[p.c() for p in problems])
    total = sum(p.H for p in problems)
    words = [p.H * ((p.n + 63) // 64) for p in problems]
    hyp = np.zeros(max(total, 1), HYPOTHESIS_DTYPE); masks = np.zeros(max(sum(words), 1), np.uint64)
    check(lib().orbm_sim3_hypotheses(arr if P else None, P, _p(sg), len(sg), _p(hyp), _p(masks)))
    out, h0, w0 = [], 0, 0
    for p, w in zip(problems, words):
        out.append((hyp[h0:h0 + p.H], masks[w0:w0 + w].reshape(p.H, (p.n + 63) // 64)))
        h0 += p.H; w0 += w
    return out


class Sim3OptProblem:
    """orbm_sim3_opt_problem: the correspondences that survive the pointer tests of Optimizer.cc:1485-1520, flat and in that order.
    cam = (fx, fy, cx, cy); R12, t12, s12: the Sim3 as LoopClosing.cc:320-325 hands it over."""

    def __init__(self, X1w, X2w, obs1, obs2, octave1, octave2, Tcw1, Tcw2, cam1, cam2, R12, t12, s12, th2, fix_scale=False):
        f = np.ascontiguousarray
        self.X1w, self.X2w = f(X1w, np.float32).reshape(-1, 3), f(X2w, np.float32).reshape(-1, 3)
        self.obs1, self.obs2 = f(obs1, np.float32).reshape(-1, 2), f(obs2, np.float32).reshape(-1, 2)
        self.octave1, self.octave2 = f(octave1, np.int32), f(octave2, np.int32)
        self.Tcw1, self.Tcw2 = f(Tcw1, np.float32).reshape(16), f(Tcw2, np.float32).reshape(16)
        self.cam1, self.cam2 = tuple(float(v) for v in cam1), tuple(float(v) for v in cam2)
        self.R12, self.t12 = f(R12, np.float32).reshape(9), f(t12, np.float32).reshape(3)
        self.s12, self.th2, self.fix_scale = float(np.float32(s12)), float(np.float32(th2)), bool(fix_scale)
        self.n = len(self.X1w)
        if not (len(self.X2w) == len(self.obs1) == len(self.obs2) == len(self.octave1) == len(self.octave2) == self.n):
            raise ValueError("X1w, X2w, obs1, obs2, octave1, octave2 differ in length")

    def c(self):
        return _CSim3OptProblem(_p(self.X1w), _p(self.X2w), _p(self.obs1), _p(self.obs2), _p(self.octave1), _p(self.octave2), _p(self.Tcw1),
                                _p(self.Tcw2), *self.cam1, *self.cam2, (C.c_float * 9)(*self.R12), (C.c_float * 3)(*self.t12), self.s12,
                                self.th2, int(self.fix_scale), self.n)


def optimize_sim3(problems, inv_level_sigma2):
    """orbm_optimize_sim3 (Optimizer::OptimizeSim3 of every problem in one launch): per problem (Sim3OptResult, kept [n] bool) --
    kept[i] where the reference leaves vpMatches1[idx] non-NULL"""
    P = len(problems)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32)
    arr = (_CSim3OptProblem * max(P, 1))(*[p.c() for p in problems])
    res = (Sim3OptResult * max(P, 1))()
    kept = np.zeros(max(sum(p.n for p in problems), 1), np.uint8)
    check(lib().orbm_optimize_sim3(arr if P else None, P, _p(sg), len(sg), res, _p(kept)))
    out, k0 = [], 0
    for i, p in enumerate(problems):
        out.append((res[i], kept[k0:k0 + p.n].astype(bool)))
        k0 += p.n
    return out


class _CRefineSim3Attempt(C.Structure):
    """orbm_refine_sim3_attempt"""
    _fields_ = [("kf2", C.c_void_p), ("points2", C.c_void_p), ("T2w", C.c_void_p), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("s12", C.c_float), ("seed12", C.c_void_p), ("found12", C.c_void_p), ("matches12", C.c_void_p)]


class RefineSim3Attempt:
    """orbm_refine_sim3_attempt: one pass of LoopClosing.cc:311-341 -- kf2 a resident Frame, points2 a Points with one entry per
    keypoint of kf2 (valid = map point non-NULL and not bad), T2w, the Sim3 as :320-325 hands it over, seed12 [n1] (>= 0 the
    point's index in KF2, -1 NULL, -2 non-NULL without an index in KF2; None: all -1)."""

    def __init__(self, kf2, points2, T2w, R12, t12, s12, seed12=None):
        f = np.ascontiguousarray
        self.kf2, self.points2 = kf2, points2
        self.T2w, self.R12, self.t12 = f(T2w, np.float32).reshape(16), f(R12, np.float32).reshape(9), f(t12, np.float32).reshape(3)
        self.s12 = float(np.float32(s12))
        self.seed12 = f(seed12, np.int32) if seed12 is not None else None


REFINE_MIN_INLIERS = 20     # LoopClosing.cc:333


def refine_sim3_candidates(kf1, points1, T1w, view, inv_level_sigma2, attempts, th=7.5, th_high=95, th2=10.0, fix_scale=False):
    """orbm_refine_sim3_candidates (SearchBySim3 chained into OptimizeSim3 for every attempt against kf1, one host wait): per attempt
    (found12 [n1], nfound, matches12 [n1], Sim3OptResult) -- found12 = what SearchBySim3 alone writes, matches12 = vpMatches1 as
    OptimizeSim3 leaves it"""
    P = len(attempts)
    sg = np.ascontiguousarray(inv_level_sigma2, np.float32)
    T1 = np.ascontiguousarray(T1w, np.float32).reshape(16)
    arr = (_CRefineSim3Attempt * max(P, 1))()
    out = []
    addr = lambda a: _p(a).value if a is not None and len(a) else None
    for c, a in zip(arr, attempts):
        found = np.full(max(kf1.n, 1), -9, np.int32); matches = np.full(max(kf1.n, 1), -9, np.int32)
        h = a.kf2._h.value if isinstance(a.kf2._h, C.c_void_p) else a.kf2._h
        c.kf2, c.points2, c.T2w = h, C.addressof(a.points2.c), addr(a.T2w)
        c.R12, c.t12, c.s12 = (C.c_float * 9)(*a.R12), (C.c_float * 3)(*a.t12), a.s12
        c.seed12, c.found12, c.matches12 = addr(a.seed12), addr(found), addr(matches)
        out.append((found, matches))
    nf = np.full(max(P, 1), -9, np.int32)
    res = (Sim3OptResult * max(P, 1))()
    check(lib().orbm_refine_sim3_candidates(kf1._h, C.byref(points1.c), _p(T1), C.byref(view.c), _p(sg), arr if P else None, P, th,
                                            int(th_high), th2, int(bool(fix_scale)), _p(nf), res))
    return [(f[:kf1.n], int(nf[p]), m[:kf1.n], res[p]) for p, (f, m) in enumerate(out)]


def first_accepted(results, min_inliers=REFINE_MIN_INLIERS):
    """the fold of the loop at LoopClosing.cc:288 over the attempts of one pass: the index of the first attempt, in order, whose
    refinement returned nin >= min_inliers, or None"""
    for p, r in enumerate(results):
        if r[3].nin >= min_inliers:
            return p
    return None


def last_refine_sim3_waits():
    """orbm_debug_last_refine_sim3_waits: host waits of the last orbm_refine_sim3_candidates call of this process."""
    return lib().orbm_debug_last_refine_sim3_waits()


def last_sim3_opt_waits():
    """orbm_debug_last_sim3_opt_waits: host waits of the last orbm_optimize_sim3 call of this process."""
    return lib().orbm_debug_last_sim3_opt_waits()


def last_sim3_waits():
    """orbm_debug_last_sim3_waits: host waits of the last orbm_sim3_hypotheses call of this process."""
    return lib().orbm_debug_last_sim3_waits()


def ransac_max_iterations(probability, min_inliers, max_iterations, N):
    """mRansacMaxIts of SetRansacParameters (:120-137)"""
    if min_inliers == N:
        n_iterations = 1
    else:
        epsilon = float(np.float32(min_inliers) / np.float32(N)) if N else math.inf
        try:
            v = math.ceil(math.log(1 - probability) / math.log(1 - epsilon ** 3))
        except (ValueError, ZeroDivisionError, OverflowError):
            # log of 0 or of a negative number: -0 (-> 0 iterations) resp. NaN (-> INT_MIN on x86); both end as 1 below
            v = 0
        n_iterations = v if -2 ** 31 <= v < 2 ** 31 else -2 ** 31
    return max(1, min(n_iterations, max_iterations))


def draw_triples(n, H, randint):
    """the draw loop of :163-177 for H iterations; randint(lo, hi) is inclusive, as DUtils::Random::RandomInt"""
    out = np.zeros((H, 3), np.int32)
    for h in range(H):
        avail = list(range(n))
        for i in range(3):
            r = randint(0, len(avail) - 1)
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Sim3Solver:
    """The reference's Sim3Solver.  The constructor takes the flat problem and a source of draws: `draw` = a callable (lo, hi) ->
    int, or `triples` = pre-drawn [H][3] (at least mRansacMaxIts rows).  indices1 = mvnIndices1 (where each kept pair stands in
    vpMatched12) and N1 = vpMatched12.size() shape vbInliers; by default the pairs are the whole vector."""

    def __init__(self, X1w, X2w, octave1, octave2, Tcw1, Tcw2, cam1, cam2, level_sigma2, fix_scale=False, draw=None, triples=None,
                 indices1=None, N1=None):
        if (draw is None) == (triples is None):
            raise ValueError("give either draw or triples")
        self._args = (X1w, X2w, octave1, octave2, Tcw1, Tcw2, cam1, cam2)
        self._sigma2, self._fix_scale, self._draw = level_sigma2, fix_scale, draw
        self._triples = None if triples is None else np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        self.N = len(np.asarray(X1w).reshape(-1, 3))
        self.mvnIndices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = self.N if N1 is None else int(N1)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = None
        self._hyp = self._masks = self.triples = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb, self.mRansacMinInliers = probability, minInliers
        self.mRansacMaxIts = ransac_max_iterations(probability, minInliers, maxIterations, self.N)
        self.mnIterations = 0
        if self.mRansacMaxIts > MAX_H:
            raise ValueError(f"more than {MAX_H} iterations")

    # ---- the first evaluation
    def _needs_evaluation(self):
        return self._hyp is None and self.N >= self.mRansacMinInliers

    def _problem(self):
        H = self.mRansacMaxIts
        tri = draw_triples(self.N, H, self._draw) if self._draw is not None else self._triples[:H]
        if len(tri) < H:
            raise ValueError("fewer pre-drawn triples than mRansacMaxIts")
        self.triples = np.ascontiguousarray(tri, np.int32)        # the draws of all iterations, as evaluated
        return Sim3Problem(*self._args, self.triples, self._fix_scale)

    @staticmethod
    def EvaluateBatch(solvers):
        """the first evaluation of all candidates of a loop detection in one orbm_sim3_hypotheses call"""
        todo = [s for s in solvers if s._needs_evaluation()]
        for k in range(0, len(todo), MAX_PROBLEMS):
            part = todo[k:k + MAX_PROBLEMS]
            sigma2 = part[0]._sigma2
            for s, (hyp, masks) in zip(part, sim3_hypotheses([s._problem() for s in part], sigma2)):
                s._hyp, s._masks = hyp.copy(), masks.copy()

    # ---- the fold of iterate (:140-207) over the stored counts
    def iterate(self, nIterations):
        """(T12 [4, 4] or None, bNoMore, vbInliers [mN1] bool, nInliers)"""
        vbInliers = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, 0
        if self._hyp is None:
            Sim3Solver.EvaluateBatch([self])
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            h = self.mnIterations
            cur += 1; self.mnIterations += 1
            cnt = int(self._hyp["ninliers"][h])
            if cnt >= self.mnBestInliers:
                self.mnBestInliers, self._best = cnt, h
                if cnt > self.mRansacMinInliers:
                    vbInliers[self.mvnIndices1[self.inlier_flags(h)]] = True
                    return self._hyp["T12"][h].reshape(4, 4).copy(), False, vbInliers, cnt
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0

    def find(self):
        """(T12 or None, vbInliers12, nInliers)"""
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n

    def inlier_flags(self, h):
        """mvbInliersi [N] of hypothesis h"""
        bits = np.unpackbits(self._masks[h].view(np.uint8), bitorder="little")
        return bits[:self.N].astype(bool)

    def GetEstimatedRotation(self):
        return self._hyp["R12"][self._best].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self._hyp["t12"][self._best].reshape(3, 1).copy()

    def GetEstimatedScale(self):
        return float(self._hyp["s12"][self._best])
