"""The projection prefix of the SearchByProjection family restated in numpy, entry by entry, with the outcome the reference
reaches for every entry.  TEST INFRASTRUCTURE ONLY.

Written from the reference lines the kernels cite: Frame::isInFrustum (src/Frame.cc:284-340) with MapPoint::PredictScale
(src/MapPoint.cc:464-480) and RadiusByViewingCos (src/ORBmatcher.cc:332-338); the projection blocks of the two Fuse forms
(:1053-1094, :1212-1250); SearchByProjection(Cur, Last) (:1529-1671), (Cur, KF) (:1673-1800), (KF, Scw) (:491-604) and the two
directions of SearchBySim3 (:1303-1527); Frame::PosInGrid / GetFeaturesInArea (src/Frame.cc:342-407) with the stereo test of
:62-96; the rotation histogram and ComputeThreeMaxima (:1802-1843).

Float work is float32 where the reference uses float, one rounding per operation.  cv::Mat arithmetic as oracle/match_oracle.c
states it: Rcw * P + tcw = the row sum in float, left to right, then float(double(sum) + double(t)); cv::norm = sqrt of the double
sum of squares; Mat::dot = the double sum of double products; -R.t() * t = float(-double(row sum)).  log of a float is the C
library's logf (called through ctypes); ceil / round of a float are exact.  Every float -> int conversion goes through f2i, which
has the x86-64 meaning (NaN or out of range: INT_MIN): the reference runs there, and C leaves the case undefined.
"""
import ctypes as C
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN = -(1 << 31)
HISTO_LENGTH = 30
GRID_COLS, GRID_ROWS = 64, 48

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]

# per-entry outcome codes, in the order the reference decides them
INVALID = 0      # no map point / bad / already found (the caller's flag)
BEHIND = 1       # PcZ < 0 (isInFrustum, Fuse, Sim3 forms) or invzc < 0 (LAST)
OUT_U = 2        # u outside the bounds (isInFrustum / LAST / KF: u < minX || u > maxX; IsInImage: !(minX <= u < maxX))
OUT_V = 3
TOO_NEAR = 4     # dist below the scale-invariance range
TOO_FAR = 5      # dist above it
VIEW_ANGLE = 6   # viewCos < limit (isInFrustum) or dot < 0.5 dist (Fuse, Sim3 forms)
ACCEPTED = 7     # radius 3.0 in isInFrustum (viewCos > 0.998), th otherwise
ACCEPTED_WIDE = 8  # isInFrustum with viewCos <= 0.998: radius 4.5
NAMES = ("invalid", "behind", "out_u", "out_v", "too_near", "too_far", "view_angle", "accepted", "accepted_wide")
# PredictScale's clamp of an accepted entry
LEVEL_IN, LEVEL_LOW, LEVEL_HIGH = 0, 1, 2

PROJ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("view_cos", "<f4"), ("dist", "<f4"), ("level", "<i4"),
                       ("visible", "<i4")])
WQ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("r", "<f4"), ("xr", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")])


def f2i(x):
    """(int)x of a float as x86-64's cvttss2si computes it."""
    x = f32(x)
    return int(x) if -2147483648.0 <= x < 2147483648.0 else INT_MIN


def logf(x):
    return f32(_libm.logf(float(x)))


def roundf(x):
    """C roundf: half away from zero (exact: |x| < 2^24 adds 0.5 exactly in double, larger floats are integers)."""
    x = f64(f32(x))
    return f32(np.copysign(np.floor(abs(x) + 0.5), x))


def _row(R, k, b, t):
    s = f32(f32(f32(R[3 * k] * b[0]) + f32(R[3 * k + 1] * b[1])) + f32(R[3 * k + 2] * b[2]))
    return f32(f64(s) + f64(t))


def gemm(R, b, t):
    """Rcw * P + tcw as cv::gemm's 3 x 3 case."""
    R = np.asarray(R, f32).reshape(9); b = np.asarray(b, f32).reshape(3); t = np.asarray(t, f32).reshape(3)
    return np.array([_row(R, k, b, t[k]) for k in range(3)], f32)


def norm3(a):
    a = np.asarray(a, f32)
    return f32(np.sqrt(f64(a[0]) * f64(a[0]) + f64(a[1]) * f64(a[1]) + f64(a[2]) * f64(a[2])))


def dot3(a, n):
    return f64(a[0]) * f64(n[0]) + f64(a[1]) * f64(n[1]) + f64(a[2]) * f64(n[2])


def neg_rt_t(R, t):
    """-R.t() * t (Ow, twc): the row sums of R^T in float, times -1.0 in double."""
    R = np.asarray(R, f32).reshape(3, 3); t = np.asarray(t, f32).reshape(3)
    Rt = R.T.reshape(9)
    out = []
    for k in range(3):
        s = f32(f32(f32(Rt[3 * k] * t[0]) + f32(Rt[3 * k + 1] * t[1])) + f32(Rt[3 * k + 2] * t[2]))
        out.append(f32(f64(s) * -1.0 + 0.0))
    return np.array(out, f32)


def pose_parts(T):
    T = np.asarray(T, f32).reshape(4, 4)
    return T[:3, :3].reshape(9).copy(), T[:3, 3].copy()


def camera_centre(T):
    R, t = pose_parts(T)
    return neg_rt_t(R, t)


def _scale(A, s):
    """convertTo(.., alpha = s): float(alpha) times each element plus float(0)."""
    a = f32(s)
    return np.array([f32(f32(x * a) + f32(0.0)) for x in np.asarray(A, f32).reshape(-1)], f32)


def decompose_sim3(S):
    """Scw -> Rcw, tcw, Ow (:500-504)."""
    sR, st = pose_parts(S)
    s = f32(np.sqrt(f64(sR[0]) * f64(sR[0]) + f64(sR[1]) * f64(sR[1]) + f64(sR[2]) * f64(sR[2])))
    R = _scale(sR, 1.0 / f64(s)); t = _scale(st, 1.0 / f64(s))
    return R, t, neg_rt_t(R, t)


def sim3_transforms(s12, R12, t12):
    """sR12, sR21, t21 (:1320-1323)."""
    R12 = np.asarray(R12, f32).reshape(3, 3)
    sR12 = _scale(R12, f64(f32(s12))); sR21 = _scale(R12.T, 1.0 / f64(f32(s12)))
    return sR12, sR21, neg_rt_t(sR21.reshape(3, 3).T, t12)


def motion_direction(Tcw, Tlw, mb, mono):
    """bForward / bBackward of :1540-1550."""
    Rcw, tcw = pose_parts(Tcw); Rlw, tlw = pose_parts(Tlw)
    tlc = gemm(Rlw, neg_rt_t(Rcw, tcw), tlw)
    return bool(tlc[2] > f32(mb) and not mono), bool(-tlc[2] > f32(mb) and not mono)


def predict_scale(maxd, dist, log_scale, nlevels):
    """MapPoint::PredictScale with the float ratio: (level, clamp code)."""
    with np.errstate(all="ignore"):
        ratio = f32(f32(maxd) / f32(dist))
        q = f32(logf(ratio) / f32(log_scale))
    n = f2i(np.ceil(q))
    if n < 0:
        return 0, LEVEL_LOW
    if n >= nlevels:
        return nlevels - 1, LEVEL_HIGH
    return n, LEVEL_IN


def project_points(mode, pos, nrm, mind, maxd, Rcw, tcw, Ow, cam4, bounds4, mbf, cos_limit, log_scale, scale_factors, th, valid=None):
    """Frame::isInFrustum + PredictScale (mode 0) / the Fuse projection blocks (1: 1 / z in float, 2: 1.0 / z in double).
    Returns (projected[PROJ_DTYPE], queries[WQ_DTYPE], code[int8], clamp[int8, -1 unless accepted])."""
    fx, fy, cx, cy = [f32(v) for v in cam4]
    minx, miny, maxx, maxy = [f32(v) for v in bounds4]
    sf = np.asarray(scale_factors, f32); nl = len(sf)
    mbf, cos_limit, th = f32(mbf), f32(cos_limit), f32(th)
    pos = np.asarray(pos, f32).reshape(-1, 3); nrm = np.asarray(nrm, f32).reshape(-1, 3)
    mind = np.asarray(mind, f32); maxd = np.asarray(maxd, f32); Ow = np.asarray(Ow, f32).reshape(3)
    m = len(pos)
    out = np.zeros(m, PROJ_DTYPE); out["level"] = -1
    q = np.zeros(m, WQ_DTYPE); q["r"] = -1; q["max_level"] = -1
    code = np.zeros(m, np.int8); clamp = np.full(m, -1, np.int8)
    with np.errstate(all="ignore"):
        for i in range(m):
            if valid is not None and not valid[i]:
                code[i] = INVALID; continue
            P = pos[i]
            X, Y, Z = gemm(Rcw, P, tcw)
            if Z < f32(0):
                code[i] = BEHIND; continue
            if mode == 0:
                invz = f32(f32(1) / Z)
                u = f32(f32(f32(fx * X) * invz) + cx); v = f32(f32(f32(fy * Y) * invz) + cy)
                if u < minx or u > maxx:
                    code[i] = OUT_U; continue
                if v < miny or v > maxy:
                    code[i] = OUT_V; continue
            else:
                invz = f32(f32(1) / Z) if mode == 1 else f32(1.0 / f64(Z))
                x, y = f32(X * invz), f32(Y * invz)
                u = f32(f32(fx * x) + cx); v = f32(f32(fy * y) + cy)
                if not (u >= minx and u < maxx):
                    code[i] = OUT_U; continue
                if not (v >= miny and v < maxy):
                    code[i] = OUT_V; continue
            ur = f32(u - f32(mbf * invz))
            maxD, minD = f32(f32(1.2) * maxd[i]), f32(f32(0.8) * mind[i])
            PO = np.array([f32(P[k] - Ow[k]) for k in range(3)], f32)
            dist = norm3(PO)
            dot = dot3(PO, nrm[i])
            view_cos = f32(0)
            if mode == 0:
                if f64(dist) < 0.9 * f64(minD):
                    code[i] = TOO_NEAR; continue
                if f64(dist) > f64(maxD) / 0.9:
                    code[i] = TOO_FAR; continue
                view_cos = f32(dot / f64(dist))
                if view_cos < cos_limit:
                    code[i] = VIEW_ANGLE; continue
            else:
                if dist < minD:
                    code[i] = TOO_NEAR; continue
                if dist > maxD:
                    code[i] = TOO_FAR; continue
                if dot < 0.5 * f64(dist):
                    code[i] = VIEW_ANGLE; continue
            level, clamp[i] = predict_scale(maxd[i], dist, log_scale, nl)
            if mode == 0:
                wide = not (f64(view_cos) > 0.998)
                r = f32(4.5) if wide else f32(3.0)
                if f64(th) != 1.0:
                    r = f32(r * th)
                code[i] = ACCEPTED_WIDE if wide else ACCEPTED
            else:
                r = th
                code[i] = ACCEPTED
            out[i] = (u, v, ur, view_cos, dist, level, 1)
            q[i] = (u, v, f32(r * sf[level]), ur, level - 1, level)
    return out, q, code, clamp


FORM_LAST, FORM_KF, FORM_SIM3, FORM_PAIR = 0, 1, 2, 3


def project_form(form, valid, pos, cam4, bounds4, scale_factors, log_scale=None, th=1.0, *, Rcw=None, tcw=None, Ow=None, mind=None,
                 maxd=None, nrm=None, octave=None, mbf=0.0, forward=False, backward=False, R2=None, t2=None):
    """The projection prefix of one whole search: LAST (:1553-1591), KF (:1700-1730), SIM3 (:521-575) or one PAIR direction of
    SearchBySim3 (:1360-1396; R2 / t2 = sR21, t21 or sR12, t12).  Returns (queries[WQ_DTYPE], code[int8], clamp[int8])."""
    fx, fy, cx, cy = [f32(v) for v in cam4]
    minx, miny, maxx, maxy = [f32(v) for v in bounds4]
    sf = np.asarray(scale_factors, f32); nl = len(sf)
    th, mbf = f32(th), f32(mbf)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    m = len(pos)
    q = np.zeros(m, WQ_DTYPE); q["r"] = -1; q["max_level"] = -1
    code = np.zeros(m, np.int8); clamp = np.full(m, -1, np.int8)
    with np.errstate(all="ignore"):
        for i in range(m):
            if not valid[i]:
                code[i] = INVALID; continue
            P = pos[i]
            X, Y, Z = gemm(Rcw, P, tcw)
            if form == FORM_LAST or form == FORM_KF:
                invzc = f32(1.0 / f64(Z))
                if form == FORM_LAST and invzc < 0:
                    code[i] = BEHIND; continue
                u = f32(f32(f32(fx * X) * invzc) + cx); v = f32(f32(f32(fy * Y) * invzc) + cy)
                if u < minx or u > maxx:
                    code[i] = OUT_U; continue
                if v < miny or v > maxy:
                    code[i] = OUT_V; continue
                if form == FORM_LAST:
                    oct_ = int(octave[i])
                    lo = oct_ if forward else (0 if backward else oct_ - 1)
                    hi = -1 if forward else (oct_ if backward else oct_ + 1)
                    q[i] = (u, v, f32(th * sf[oct_]), f32(u - f32(mbf * invzc)), lo, hi)
                    code[i] = ACCEPTED; continue
                PO = np.array([f32(P[k] - Ow[k]) for k in range(3)], f32)
                dist = norm3(PO)
                if dist < f32(f32(0.8) * f32(mind[i])):
                    code[i] = TOO_NEAR; continue
                if dist > f32(f32(1.2) * f32(maxd[i])):
                    code[i] = TOO_FAR; continue
                level, clamp[i] = predict_scale(maxd[i], dist, log_scale, nl)
                q[i] = (u, v, f32(th * sf[level]), f32(0), level - 1, level + 1)
                code[i] = ACCEPTED; continue
            if form == FORM_PAIR:
                X, Y, Z = gemm(R2, np.array([X, Y, Z], f32), t2)
            if Z < f32(0):
                code[i] = BEHIND; continue
            invz = f32(f32(1) / Z) if form == FORM_SIM3 else f32(1.0 / f64(Z))
            x, y = f32(X * invz), f32(Y * invz)
            u = f32(f32(fx * x) + cx); v = f32(f32(fy * y) + cy)
            if not (u >= minx and u < maxx):
                code[i] = OUT_U; continue
            if not (v >= miny and v < maxy):
                code[i] = OUT_V; continue
            maxD, minD = f32(f32(1.2) * f32(maxd[i])), f32(f32(0.8) * f32(mind[i]))
            if form == FORM_SIM3:
                PO = np.array([f32(P[k] - Ow[k]) for k in range(3)], f32)
                dist = norm3(PO)
            else:
                dist = norm3(np.array([X, Y, Z], f32))
            if dist < minD:
                code[i] = TOO_NEAR; continue
            if dist > maxD:
                code[i] = TOO_FAR; continue
            if form == FORM_SIM3 and dot3(PO, np.asarray(nrm, f32).reshape(-1, 3)[i]) < 0.5 * f64(dist):
                code[i] = VIEW_ANGLE; continue
            level, clamp[i] = predict_scale(maxd[i], dist, log_scale, nl)
            q[i] = (u, v, f32(th * sf[level]), f32(0), level - 1, level)
            code[i] = ACCEPTED
    return q, code, clamp


def form_last(Tcw, Tlw, valid, pos, octave, cam4, bounds4, scale_factors, mb, mbf, th, mono):
    R, t = pose_parts(Tcw)
    fwd, bwd = motion_direction(Tcw, Tlw, mb, mono)
    return project_form(FORM_LAST, valid, pos, cam4, bounds4, scale_factors, th=th, Rcw=R, tcw=t, octave=octave, mbf=mbf,
                        forward=fwd, backward=bwd)


def form_kf(Tcw, valid, pos, mind, maxd, cam4, bounds4, scale_factors, log_scale, th):
    R, t = pose_parts(Tcw)
    return project_form(FORM_KF, valid, pos, cam4, bounds4, scale_factors, log_scale, th, Rcw=R, tcw=t, Ow=neg_rt_t(R, t),
                        mind=mind, maxd=maxd)


def form_sim3(Scw, valid, pos, nrm, mind, maxd, cam4, bounds4, scale_factors, log_scale, th):
    R, t, Ow = decompose_sim3(Scw)
    return project_form(FORM_SIM3, valid, pos, cam4, bounds4, scale_factors, log_scale, f32(int(th)), Rcw=R, tcw=t, Ow=Ow,
                        mind=mind, maxd=maxd, nrm=nrm)


def form_pair(T1w, T2w, s12, R12, t12, valid1, pos1, mind1, maxd1, valid2, pos2, mind2, maxd2, cam4, bounds4, scale_factors,
              log_scale, th):
    """Both directions of SearchBySim3: (q12, code12, clamp12), (q21, code21, clamp21)."""
    sR12, sR21, t21 = sim3_transforms(s12, R12, t12)
    R1, t1 = pose_parts(T1w); R2, t2 = pose_parts(T2w)
    a = project_form(FORM_PAIR, valid1, pos1, cam4, bounds4, scale_factors, log_scale, th, Rcw=R1, tcw=t1, mind=mind1, maxd=maxd1,
                     R2=sR21, t2=t21)
    b = project_form(FORM_PAIR, valid2, pos2, cam4, bounds4, scale_factors, log_scale, th, Rcw=R2, tcw=t2, mind=mind2, maxd=maxd2,
                     R2=sR12, t2=np.asarray(t12, f32).reshape(3))
    return a, b


# ------------------------------------------------------------------------------------------------------------ the grid window
W_IN, W_LEVEL, W_DX, W_DY, W_OCCUPIED, W_URIGHT = 0, 1, 2, 3, 4, 5
W_NAMES = ("in", "level", "dx", "dy", "occupied", "uright")


class Grid:
    """Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:245-260, 397-407) of keypoints x, y in the bounds' cell pitch."""

    def __init__(self, x, y, bounds4, query_bounds4=None):
        minx, miny, maxx, maxy = [f32(v) for v in bounds4]
        self.inv_w = f32(f32(GRID_COLS) / f32(maxx - minx)); self.inv_h = f32(f32(GRID_ROWS) / f32(maxy - miny))
        qb = query_bounds4 if query_bounds4 is not None else bounds4
        self.min_x, self.min_y = f32(qb[0]), f32(qb[1])
        self.x = np.asarray(x, f32); self.y = np.asarray(y, f32)
        self.cells = [[] for _ in range(GRID_COLS * GRID_ROWS)]
        self.cell = np.full(len(self.x), -1, np.int64)
        with np.errstate(all="ignore"):
            for j in range(len(self.x)):
                px = f2i(roundf(f32(f32(self.x[j] - minx) * self.inv_w)))
                py = f2i(roundf(f32(f32(self.y[j] - miny) * self.inv_h)))
                if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
                    self.cell[j] = px * GRID_ROWS + py
                    self.cells[px * GRID_ROWS + py].append(j)

    def layout(self):
        """(perm, cell_off): keypoints in (cell, index) order, as orbm_sorted_frame reports them."""
        perm = [j for c in self.cells for j in c]
        off = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32); off[1:] = np.cumsum([len(c) for c in self.cells])
        return np.array(perm, np.int32), off

    def window(self, x, y, r, min_level, max_level, octave, occupied=None, uright=None, xr=None):
        """GetFeaturesInArea (:342-395) + the occupancy and stereo tests of the search loops: [(j, reason)] for every keypoint
        of the scanned cells, in the order the reference visits them (reason W_IN: a candidate)."""
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        with np.errstate(all="ignore"):
            c0 = f2i(np.fmax(f32(0), np.floor(f32(f32(f32(x - self.min_x) - r) * self.inv_w))))
            if c0 >= GRID_COLS:
                return out
            c1 = f2i(np.fmin(f32(GRID_COLS - 1), np.ceil(f32(f32(f32(x - self.min_x) + r) * self.inv_w))))
            if c1 < 0:
                return out
            r0 = f2i(np.fmax(f32(0), np.floor(f32(f32(f32(y - self.min_y) - r) * self.inv_h))))
            if r0 >= GRID_ROWS:
                return out
            r1 = f2i(np.fmin(f32(GRID_ROWS - 1), np.ceil(f32(f32(f32(y - self.min_y) + r) * self.inv_h))))
            if r1 < 0:
                return out
            check = min_level > 0 or max_level >= 0
            for ix in range(c0, c1 + 1):
                for iy in range(r0, r1 + 1):
                    for j in self.cells[ix * GRID_ROWS + iy]:
                        o = int(octave[j])
                        if check and (o < min_level or (max_level >= 0 and o > max_level)):
                            out.append((j, W_LEVEL)); continue
                        if not abs(f32(self.x[j] - x)) < r:
                            out.append((j, W_DX)); continue
                        if not abs(f32(self.y[j] - y)) < r:
                            out.append((j, W_DY)); continue
                        if occupied is not None and occupied[j]:
                            out.append((j, W_OCCUPIED)); continue
                        if uright is not None and uright[j] > 0 and abs(f32(f32(xr) - f32(uright[j]))) > r:
                            out.append((j, W_URIGHT)); continue
                        out.append((j, W_IN))
        return out


# ------------------------------------------------------------------------------------------------------------ the rotation rule
def rot_bin(a1, a2):
    """The bin of a match's angle difference (e.g. :1640-1647): round(rot / 30 ...) with factor = 1.0f / HISTO_LENGTH."""
    rot = f32(f32(a1) - f32(a2))
    if rot < f32(0):
        rot = f32(rot + f32(360))
    b = f2i(roundf(f32(rot * f32(f32(1) / f32(HISTO_LENGTH)))))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(hist):
    """ComputeThreeMaxima (:1802-1843): (ind1, ind2, ind3), -1 for none."""
    max1 = max2 = max3 = 0; ind1 = ind2 = ind3 = -1
    for i, s in enumerate(int(v) for v in hist):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif f32(max3) < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3
