"""PnPsolver (src/PnPsolver.cc) over orbm_pnp_hypotheses: the reference's interface, with every EPnP RANSAC hypothesis of one or
several candidate keyframes -- compute_pose, CheckInliers and the Refine behind every new best -- evaluated on the device in one
call, and iterate() as the reference's fold over the stored results.

One difference to the reference: the draws of one solver are made together, when its hypotheses are evaluated; in
Tracking::Relocalization they interleave with the other candidates' draws in five-iteration rounds.  Results equal the reference
run whose RNG hands each solver these sets (the reference seeds nothing here).  The arithmetic is the reference's in IEEE double
with one stated departure, the SVD's hypot."""
import ctypes as C
import math

import numpy as np

from ._lib import check, lib, ptr as _p


class _CPnpProblem(C.Structure):
    """orbm_pnp_problem"""
    _fields_ = [("Xw", C.c_void_p), ("uv", C.c_void_p), ("octave", C.c_void_p), ("sets", C.c_void_p), ("fu", C.c_double), ("fv", C.c_double),
                ("uc", C.c_double), ("vc", C.c_double), ("th2", C.c_float), ("n", C.c_int32), ("H", C.c_int32), ("min_inliers", C.c_int32)]


HYPOTHESIS_DTYPE = np.dtype([("R", "f8", 9), ("t", "f8", 3), ("rep_error", "f8"), ("ninliers", "i4"), ("refined", "i4"), ("Rr", "f8", 9),
                             ("tr", "f8", 3), ("nrefined", "i4"), ("pad", "i4")])   # orbm_pnp_hypothesis

MAX_PROBLEMS, MAX_N, MAX_H = 64, 8192, 1024


class PnpProblem:
    """orbm_pnp_problem: what the reference's constructor keeps (:81-103), flat.  cam = (fu, fv, uc, vc); min_inliers =
    mRansacMinInliers after SetRansacParameters."""

    def __init__(self, Xw, uv, octave, cam, sets, min_inliers, th2=5.991):
        f = np.ascontiguousarray
        self.Xw, self.uv = f(Xw, np.float32).reshape(-1, 3), f(uv, np.float32).reshape(-1, 2)
        self.octave, self.sets = f(octave, np.int32), f(sets, np.int32).reshape(-1, 4)
        self.cam = tuple(float(v) for v in cam)
        self.th2, self.min_inliers = float(np.float32(th2)), int(min_inliers)
        self.n, self.H = len(self.Xw), len(self.sets)
        if not (len(self.uv) == len(self.octave) == self.n):
            raise ValueError("Xw, uv, octave differ in length")

    def c(self):
        return _CPnpProblem(_p(self.Xw), _p(self.uv), _p(self.octave), _p(self.sets), *self.cam, self.th2, self.n, self.H, self.min_inliers)


def pnp_hypotheses(problems, level_sigma2, best_in=None):
    """orbm_pnp_hypotheses: per problem (hyp [H] of HYPOTHESIS_DTYPE, masks [H, (n + 63) // 64] uint64, refined masks, the same shape)"""
    P = len(problems)
    sg = np.ascontiguousarray(level_sigma2, np.float32)
    arr = (_CPnpProblem * max(P, 1))(*[p.c() for p in problems])
    total = sum(p.H for p in problems)
    words = [p.H * ((p.n + 63) // 64) for p in problems]
    hyp = np.zeros(max(total, 1), HYPOTHESIS_DTYPE)
    masks, rmasks = np.zeros(max(sum(words), 1), np.uint64), np.zeros(max(sum(words), 1), np.uint64)
    best = None if best_in is None else np.ascontiguousarray(best_in, np.int32)
    if best is not None and len(best) != P:
        raise ValueError("best_in needs one entry per problem")
    check(lib().orbm_pnp_hypotheses(arr if P else None, P, _p(sg), len(sg), None if best is None or P == 0 else _p(best), _p(hyp), _p(masks),
                                    _p(rmasks)))
    out, h0, w0 = [], 0, 0
    for p, w in zip(problems, words):
        shape = (p.H, (p.n + 63) // 64)
        out.append((hyp[h0:h0 + p.H], masks[w0:w0 + w].reshape(shape), rmasks[w0:w0 + w].reshape(shape)))
        h0 += p.H; w0 += w
    return out


def last_pnp_waits():
    """orbm_debug_last_pnp_waits: host waits of the last orbm_pnp_hypotheses call of this process."""
    return lib().orbm_debug_last_pnp_waits()


def pnp_pose(pws, us, cam):
    """orbm_debug_pnp_pose (test aid): compute_pose of n = 4 .. 2,048 correspondences in double on the host -> (R [3, 3], t [3], rep_error)"""
    pws = np.ascontiguousarray(pws, np.float64).reshape(-1, 3); us = np.ascontiguousarray(us, np.float64).reshape(-1, 2)
    if len(pws) != len(us):
        raise ValueError("pws, us differ in length")
    cam = np.ascontiguousarray(cam, np.float64)
    R, t, rep = np.zeros((3, 3)), np.zeros(3), np.zeros(1)
    check(lib().orbm_debug_pnp_pose(_p(pws), _p(us), len(pws), _p(cam), _p(R), _p(t), _p(rep)))
    return R, t, float(rep[0])


def ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
    """SetRansacParameters (:123-159) -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)"""
    f32 = np.float32
    eps = f32(epsilon)
    n_min = int(f32(N) * eps)                                          # int nMinInliers = N * mRansacEpsilon
    n_min = max(n_min, minInliers, minSet)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = f32(n_min) / f32(N)
    if eps < ratio:
        eps = ratio
    if n_min == N:
        n_iterations = 1
    else:
        try:
            v = math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3))
        except (ValueError, ZeroDivisionError, OverflowError):
            # log of 0 or of a negative number: -0 (-> 0 iterations) resp. NaN (-> INT_MIN on x86); both end as 1 below
            v = 0
        n_iterations = v if -2 ** 31 <= v < 2 ** 31 else -2 ** 31
    return n_min, max(1, min(n_iterations, maxIterations)), float(eps)


def draw_sets(n, H, randint, frame_rule=False):
    """the draw loop of :193-206 for H iterations; randint(lo, hi) is inclusive, as DUtils::Random::RandomInt.  frame_rule: the
    loop of iterate(Frame &, ..) (:304-317), which overwrites element [idx] of its list instead of element [randi] and can
    therefore draw a correspondence twice (a write past the list's current end lands in the vector's spare capacity)."""
    out = np.zeros((H, 4), np.int32)
    for h in range(H):
        avail, size = list(range(n)), n
        for i in range(4):
            r = randint(0, size - 1)
            idx = avail[r]
            out[h, i] = idx
            avail[idx if frame_rule else r] = avail[size - 1]
            size -= 1
    return out


def _flags(mask_row, n):
    return np.unpackbits(np.ascontiguousarray(mask_row).view(np.uint8), bitorder="little")[:n].astype(bool)


def _tcw(R, t):
    """the float conversion of mRi, mti into a 4 x 4 (:223-229)"""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3).astype(np.float32)
    T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


class PnPsolver:
    """The reference's PnPsolver.  The constructor takes the flat problem and a source of draws: `draw` = a callable (lo, hi) ->
    int, or `sets` = pre-drawn [H][4], consumed in order.  indices = mvKeyPointIndices (where each kept correspondence stands in
    vpMapPointMatches) and n_matches = vpMapPointMatches.size() shape vbInliers; by default the correspondences are the whole vector."""

    def __init__(self, Xw, uv, octave, cam, level_sigma2, draw=None, sets=None, indices=None, n_matches=None):
        if (draw is None) == (sets is None):
            raise ValueError("give either draw or sets")
        self._Xw, self._uv, self._octave, self._cam = Xw, uv, octave, cam
        self._sigma2, self._draw = np.ascontiguousarray(level_sigma2, np.float32), draw
        self._sets = None if sets is None else np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
        self._drawn = np.zeros((0, 4), np.int32)                      # the sets of all iterations so far, as evaluated
        self.N = len(np.asarray(Xw).reshape(-1, 3))
        self.mvKeyPointIndices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self.n_matches = self.N if n_matches is None else int(n_matches)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = None                                             # (R, t, flags) of mBestTcw / mvbBestInliers
        self._last_refined = 0                                        # mnRefinedInliers of the last Refine()
        self._refined = None                                          # (Rr, tr, flags) of that Refine()
        self._start, self._hyp, self._masks, self._rmasks = 0, None, None, None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        if minSet != 4:
            raise ValueError("the set size is 4, the only value the reference passes")
        self.mRansacProb, self.mRansacMinSet, self.th2 = probability, minSet, th2
        self.mRansacMinInliers, self.mRansacMaxIts, self.mRansacEpsilon = ransac_parameters(self.N, probability, minInliers, maxIterations, minSet,
                                                                                             epsilon)
        octave = np.asarray(self._octave, np.int64)
        self.mvMaxError = self._sigma2[octave] * np.float32(th2)
        self._hyp = None                                              # min_inliers decides the records: evaluate again

    # ---- evaluation of the hypotheses [start, stop)
    def _sets_for(self, start, stop, frame_rule=False):
        if self._draw is not None:
            if len(self._drawn) < stop:
                self._drawn = np.concatenate([self._drawn, draw_sets(self.N, stop - len(self._drawn), self._draw, frame_rule)])
            return self._drawn[start:stop]
        if len(self._sets) < stop:
            raise ValueError("fewer pre-drawn sets than iterations")
        return self._sets[start:stop]

    def _covered(self, start, stop):
        return self._hyp is not None and self._start <= start and stop <= self._start + len(self._hyp)

    def _problem(self, start, stop, frame_rule=False):
        if stop - start > MAX_H:
            raise ValueError(f"more than {MAX_H} iterations in one evaluation")
        return PnpProblem(self._Xw, self._uv, self._octave, self._cam, self._sets_for(start, stop, frame_rule), self.mRansacMinInliers, self.th2)

    def _store(self, start, result):
        hyp, masks, rmasks = result
        self._start, self._hyp, self._masks, self._rmasks = start, hyp.copy(), masks.copy(), rmasks.copy()

    def _span(self, nIterations):
        """how many iterations the loop condition of :187 runs when nothing returns early"""
        return max(self.mRansacMaxIts - self.mnIterations, nIterations, 0)

    @staticmethod
    def evaluate(solvers, nIterations=5):
        """the evaluation that each solver's next iterate(nIterations) needs, for all candidates of a relocalisation in one
        orbm_pnp_hypotheses call (the first iterate of a solver runs every iteration up to mRansacMaxIts)"""
        todo = []
        for s in solvers:
            a, b = s.mnIterations, s.mnIterations + s._span(nIterations)
            if s.N >= s.mRansacMinInliers and b > a and not s._covered(a, b):
                todo.append((s, a, b))
        for k in range(0, len(todo), MAX_PROBLEMS):
            part = todo[k:k + MAX_PROBLEMS]
            results = pnp_hypotheses([s._problem(a, b) for s, a, b in part], part[0][0]._sigma2, [s.mnBestInliers for s, _, _ in part])
            for (s, a, _), res in zip(part, results):
                s._store(a, res)

    # ---- the fold of iterate (:170-263) over the stored results
    def iterate(self, nIterations):
        """(Tcw [4, 4] float32 or None, bNoMore, vbInliers [n_matches] bool, nInliers)"""
        vbInliers = np.zeros(self.n_matches, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, 0
        PnPsolver.evaluate([self], nIterations)
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:
            k = self.mnIterations - self._start
            cur += 1; self.mnIterations += 1
            h = self._hyp[k]
            cnt = int(h["ninliers"])
            if cnt >= self.mRansacMinInliers:
                if cnt > self.mnBestInliers:
                    # a record here is a record on the device: both start from the same mnBestInliers and walk the same counts
                    assert h["refined"] == 1
                    self.mnBestInliers = cnt
                    self._best = (h["R"].copy(), h["t"].copy(), _flags(self._masks[k], self.N))
                    self._last_refined = int(h["nrefined"])
                    self._refined = (h["Rr"].copy(), h["tr"].copy(), _flags(self._rmasks[k], self.N))
                # Refine() on an unchanged mvbBestInliers repeats its last result
                if self._last_refined > self.mRansacMinInliers:
                    vbInliers[self.mvKeyPointIndices[self._refined[2]]] = True
                    return _tcw(self._refined[0], self._refined[1]), False, vbInliers, self._last_refined
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers and self._best is not None:
                vbInliers[self.mvKeyPointIndices[self._best[2]]] = True
                return _tcw(self._best[0], self._best[1]), True, vbInliers, self.mnBestInliers
            return None, True, vbInliers, 0
        return None, False, vbInliers, 0

    def find(self):
        """(Tcw or None, vbInliers, nInliers)"""
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n

    # ---- the first stage of iterate(Frame &, .., Map *) (:267-416)
    def iterate_frame_stage1(self, nIterations, accept):
        """The fork's iterate up to :401, as a fold over one evaluation: mnIterations restarts at 0, the sets are drawn with the
        fork's own erase rule, every pose with 2 < inliers < mRansacMinInliers is recorded, and accept(R [3, 3], t [3]) -- the
        caller's SearchByProjection of the whole map with the refined pose, true for nMatched >= 12 -- decides a successful Refine.
        Returns (Tcw or None, vbInliers, nInliers, poses) with poses = [(R, t, ninliers, iteration)] for the second stage."""
        self.mnIterations = 0
        if self._draw is not None:
            self._drawn = np.zeros((0, 4), np.int32)
        total = max(self.mRansacMaxIts, nIterations)
        res = pnp_hypotheses([self._problem(0, total, frame_rule=True)], self._sigma2, [self.mnBestInliers])[0]
        self._store(0, res)
        vbInliers, poses, verdict = np.zeros(self.n_matches, bool), [], None
        for k in range(total):
            self.mnIterations += 1
            h = self._hyp[k]
            cnt = int(h["ninliers"])
            if 2 < cnt < self.mRansacMinInliers:
                poses.append((h["R"].reshape(3, 3).copy(), h["t"].copy(), cnt, k))
            if cnt >= self.mRansacMinInliers:
                if cnt > self.mnBestInliers:
                    self.mnBestInliers = cnt
                    self._best = (h["R"].copy(), h["t"].copy(), _flags(self._masks[k], self.N))
                    self._last_refined = int(h["nrefined"])
                    self._refined = (h["Rr"].copy(), h["tr"].copy(), _flags(self._rmasks[k], self.N))
                    verdict = None
                if self._last_refined > self.mRansacMinInliers:
                    if verdict is None:                               # the same pose gives the same search
                        verdict = bool(accept(self._refined[0].reshape(3, 3).copy(), self._refined[1].copy()))
                    if verdict:
                        vbInliers[self.mvKeyPointIndices[self._refined[2]]] = True
                        return _tcw(self._refined[0], self._refined[1]), vbInliers, self._last_refined, poses
        return None, vbInliers, 0, poses
