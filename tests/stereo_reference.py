"""Frame::ComputeStereoMatches (src/Frame.cc:527-701) restated in numpy, written from the reference function, with the
outcome of every left keypoint.  TEST INFRASTRUCTURE ONLY.

Float work is float32 where the reference uses float (minU / maxU, deltaR, bestuR, disparity, depth, thDist); the 11 x 11
L1 norms are sums of integer-valued floats below 2^24, hence exact integers.  Inputs are what the reference reads: the
left / right keypoints and descriptors, both UNPADDED pyramids (mvImagePyramid[level], OrbOracle.level_image), the scale
factors and their inverses, mb and mbf.  A correlation window that leaves the level image raises: the reference's
cv::Mat::rowRange / colRange would fail there as well.
"""
import numpy as np

# per-keypoint outcome codes, in the order the reference decides them
NO_CANDIDATE = 0     # empty row list, maxU < 0, or no right keypoint within +-1 octave and [minU, maxU]      (:569-596)
HAMMING = 1          # best Hamming distance >= thOrbDist = 70                                                (:612)
BORDER = 2           # iniu < 0 or endu >= cols of the level                                                  (:634-636)
EDGE_SHIFT = 3       # the L1 minimum at incR = -L or +L                                                      (:656-657)
DELTA = 4            # |deltaR| > 1 after the parabola fit                                                    (:666-669)
RANGE = 5            # disparity outside [minD, maxD)                                                         (:676)
CLAMPED = 6          # disparity 0 clamped to 0.01, kept by the median cut                                    (:678-682)
MEDIAN_CUT = 7       # accepted, then discarded by the median cut                                             (:687-700)
ACCEPTED = 8
NAMES = ("no_candidate", "hamming", "border", "edge_shift", "delta", "range", "clamped", "median_cut", "accepted")

TH_HIGH, TH_LOW = 95, 45
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32


def _round(v):
    """C round() of a float: half away from zero (v is a float32; exact in float64)."""
    v = float(v)
    return f32(np.copysign(np.floor(abs(v) + 0.5), v))


def stereo_matches(kL, dL, kR, dR, pyrL, pyrR, scale_factors, inv_scale_factors, mb, mbf):
    """Returns a dict: uRight, depth (float32 [N]), code (int8 [N], the constants above), nd (matches before the cut),
    median (None when nd == 0), thDist, longest_row (the longest vRowIndices list), rows (the list lengths per row),
    best_right (the Hamming match, -1 before it), unique_min (the 11 L1 distances have one minimum)."""
    sf = np.asarray(scale_factors, f32); isf = np.asarray(inv_scale_factors, f32)
    mb, mbf = f32(mb), f32(mbf)
    N, Nr = len(kL), len(kR)
    uRight = np.full(N, -1.0, f32); depth = np.full(N, -1.0, f32); code = np.full(N, -1, np.int8)
    best_right = np.full(N, -1, np.int64); unique_min = np.zeros(N, bool)
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyrL[0].shape[0]
    # row table (:537-554): right keypoint iR in every row floor(y - r) .. ceil(y + r), r = 2 scale[octave]
    rows = [[] for _ in range(nRows)]
    for iR in range(Nr):
        kpY = f32(kR["y"][iR]); r = f32(2.0) * sf[kR["octave"][iR]]
        maxr, minr = int(np.ceil(f32(kpY + r))), int(np.floor(f32(kpY - r)))
        for yi in range(max(minr, 0), min(maxr, nRows - 1) + 1):   # (rows outside the image: the reference writes out of range)
            rows[yi].append(iR)
    rows = [np.array(r, np.int64) for r in rows]
    minZ = mb; minD = f32(0.0); maxD = f32(mbf / minZ)
    octR = np.asarray(kR["octave"], np.int64); xR = np.asarray(kR["x"], f32)
    dR = np.asarray(dR, np.uint8); dL = np.asarray(dL, np.uint8)
    vDistIdx = []
    for iL in range(N):
        levelL = int(kL["octave"][iL]); vL = f32(kL["y"][iL]); uL = f32(kL["x"][iL])
        cand = rows[int(vL)]                                       # vRowIndices[vL]: float -> size_t truncates
        minU = f32(uL - maxD); maxU = f32(uL - minD)
        if len(cand) == 0 or maxU < 0:
            code[iL] = NO_CANDIDATE; continue
        ok = (octR[cand] >= levelL - 1) & (octR[cand] <= levelL + 1)
        ok &= (xR[cand] >= minU) & (xR[cand] <= maxU)
        cand = cand[ok]
        if len(cand) == 0:
            code[iL] = NO_CANDIDATE; continue
        dist = _POP[dR[cand] ^ dL[iL]].sum(1)
        bestDist, bestIdxR = TH_HIGH, 0
        j = int(np.argmin(dist))                                   # first of the minima: strict < in candidate order
        if dist[j] < bestDist:
            bestDist, bestIdxR = int(dist[j]), int(cand[j])
        if not bestDist < thOrbDist:
            code[iL] = HAMMING; continue
        best_right[iL] = bestIdxR
        uR0 = f32(kR["x"][bestIdxR])
        scaleFactor = isf[levelL]
        scaleduL = _round(f32(uL * scaleFactor)); scaledvL = _round(f32(vL * scaleFactor)); scaleduR0 = _round(f32(uR0 * scaleFactor))
        w = L = 5
        IL_img, IR_img = pyrL[levelL], pyrR[levelL]
        yl, xl, xr = int(scaledvL), int(scaleduL), int(scaleduR0)
        iniu = f32(scaleduR0 + L - w); endu = f32(scaleduR0 + L + w + 1)
        if iniu < 0 or endu >= IR_img.shape[1]:
            code[iL] = BORDER; continue
        if not (yl - w >= 0 and yl + w < IL_img.shape[0] and xl - w >= 0 and xl + w < IL_img.shape[1] and xr - L - w >= 0):
            raise AssertionError(f"keypoint {iL}: correlation window outside level {levelL}")
        IL = IL_img[yl - w:yl + w + 1, xl - w:xl + w + 1].astype(np.int64)
        IL = IL - IL[w, w]
        vDists = np.zeros(2 * L + 1, f32)
        best, bestincR = np.iinfo(np.int32).max, 0
        for incR in range(-L, L + 1):
            IR = IR_img[yl - w:yl + w + 1, xr + incR - w:xr + incR + w + 1].astype(np.int64)
            IR = IR - IR[w, w]
            d = f32(np.abs(IL - IR).sum())                         # cv::norm(NORM_L1): exact
            if d < f32(best):
                best, bestincR = int(d), incR
            vDists[L + incR] = d
        unique_min[iL] = int((vDists == vDists.min()).sum()) == 1
        if bestincR == -L or bestincR == L:
            code[iL] = EDGE_SHIFT; continue
        dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
        deltaR = f32(f32(dist1 - dist3) / f32(f32(2.0) * f32(f32(dist1 + dist3) - f32(f32(2.0) * dist2))))
        if deltaR < -1 or deltaR > 1:
            code[iL] = DELTA; continue
        bestuR = f32(sf[levelL] * f32(f32(scaleduR0 + f32(bestincR)) + deltaR))
        disparity = f32(uL - bestuR)
        if not (disparity >= minD and disparity < maxD):
            code[iL] = RANGE; continue
        clamped = disparity <= 0
        if clamped:
            disparity = f32(0.01); bestuR = f32(np.float64(uL) - 0.01)
        depth[iL] = f32(mbf / disparity)
        uRight[iL] = bestuR
        code[iL] = CLAMPED if clamped else ACCEPTED
        vDistIdx.append((best, iL))
    out = dict(nd=len(vDistIdx), median=None, thDist=None, rows=np.array([len(r) for r in rows]),
               longest_row=max((len(r) for r in rows), default=0))
    if vDistIdx:                                                   # (the reference reads vDistIdx[0] of an empty vector)
        vDistIdx.sort()
        median = f32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = f32(f32(f32(1.5) * f32(1.4)) * median)
        for dist, iL in reversed(vDistIdx):
            if f32(dist) < thDist:
                break
            uRight[iL] = -1; depth[iL] = -1; code[iL] = MEDIAN_CUT
        out.update(median=median, thDist=thDist)
    out.update(uRight=uRight, depth=depth, code=code, best_right=best_right, unique_min=unique_min)
    return out


def from_oracle(oL, oR, kL, dL, kR, dR, mb, mbf):
    """The restatement on what two OrbOracle objects just extracted (their unpadded pyramids)."""
    nl = oL.nlevels
    pyr = lambda o: [o.level_image(l)[:o.level_dims(l)[1], :o.level_dims(l)[0]] for l in range(nl)]
    sf = np.array(oL.scale_factors(), f32)
    return stereo_matches(kL, dL, kR, dR, pyr(oL), pyr(oR), sf, (f32(1.0) / sf).astype(f32), mb, mbf)
