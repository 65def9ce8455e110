"""GPU parity at the edges of the gated scan that SearchForTriangulation's three entry families share (orbm_triang.hip): lists
longer than one pass of the 16-lane stride, the winner in the first, second and last pass, an equal-distance duplicate behind it
(the reference keeps the LAST of equal distances), empty lists, and keypoint counts around the 16 keypoints of a 256-thread block.
Every result is compared with the oracle's literal loops, and the oracle's result with the constructed expectation, so that no case
passes on empty results."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from orb_slam2_e_amd import KP_DTYPE, Frame, ORBmatcher

# (list length L, position pa of the true match, position pb of its exact duplicate)
LISTS = [(0, None, None), (1, 0, None), (15, 14, None), (16, 0, 15), (17, 0, 16), (17, 15, 16), (33, 3, 32), (33, 16, 32), (48, 31, 47)]
N1 = [1, 15, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def _case(n1, L, pa, pb):
    """Keypoint i of KF1 is its own vocabulary node; node i of KF2 holds features i*L .. i*L+L-1: random fillers, the true match
    at pa and its duplicate at pb.  Geometry of test_gpu_match._triangulation_case without pixel noise; nothing owns a point, all
    mono.  Returns the inputs, the oracle's results (computed once, read-only) and the expected winners."""
    rng = np.random.default_rng(1000 * n1 + L)
    fx = fy = 500.0; cx, cy = 320.0, 240.0
    X = np.stack([rng.uniform(-2, 2, n1), rng.uniform(-1.5, 1.5, n1), rng.uniform(4, 10, n1)], 1)
    t = np.array([0.3, 0.02, 0.05])
    proj = lambda P: np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1)
    p1, p2 = proj(X), proj(X - t)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F12 = (np.linalg.inv(K).T @ tx @ np.linalg.inv(K)).astype(np.float32)
    C2 = -t; ex = np.float32(fx * C2[0] / C2[2] + cx); ey = np.float32(fy * C2[1] / C2[2] + cy)
    n2 = n1 * L
    k1 = np.zeros(n1, KP_DTYPE); k2 = np.zeros(n2, KP_DTYPE)
    k1["x"], k1["y"] = p1[:, 0], p1[:, 1]
    k1["octave"] = rng.integers(0, 8, n1); k1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    k2["x"], k2["y"] = rng.uniform(10, 630, n2), rng.uniform(10, 470, n2)                  # the fillers
    k2["octave"] = rng.integers(0, 8, n2); k2["angle"] = rng.uniform(0, 360, n2).astype(np.float32)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    flips = np.packbits(rng.random((n1, 256)) < 0.04, axis=1, bitorder="little")
    for pos in (p for p in (pa, pb) if p is not None):
        j = np.arange(n1) * L + pos
        k2["x"][j], k2["y"][j], k2["octave"][j], k2["angle"][j] = p2[:, 0], p2[:, 1], k1["octave"], k1["angle"]
        d2[j] = d1 ^ flips
    fv1 = oracle.feature_vector(np.arange(n1)); fv2 = oracle.feature_vector(np.repeat(np.arange(n1), L))
    off = (np.arange(n1 + 1) * L).astype(np.int32); idx = np.arange(n2, dtype=np.int32)
    z1 = np.zeros(n1, bool); z2 = np.zeros(n2, bool)
    sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32); sg = (sf * sf).astype(np.float32)
    if L:
        want = (np.arange(n1) * L + (pb if pb is not None else pa)).astype(np.int32)
        want_dist = np.unpackbits(flips, axis=1).sum(1).astype(np.int32)
    else:
        want = np.full(n1, -1, np.int32); want_dist = np.full(n1, ORBmatcher.TH_LOW, np.int32)
    ref_inner = oracle.match_triangulation(k1, d1, k2, d2, off, idx, z1, z2, z1, z2, F12, ex, ey, sf, sg, only_stereo=False)
    ref_whole = {ori: oracle.search_for_triangulation(k1, d1, fv1, z1, z1, k2, d2, fv2, z2, z2, F12, ex, ey, sf, sg, False, ori)
                 for ori in (False, True)}
    for a in (k1, d1, k2, d2, off, idx, z1, z2, F12, sf, sg, want, want_dist, *ref_inner, *fv1, *fv2, *(r[0] for r in ref_whole.values())):
        a.setflags(write=False)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, fv1=fv1, fv2=fv2, off=off, idx=idx, z1=z1, z2=z2, F12=F12, ex=ex, ey=ey, sf=sf, sg=sg,
                want=want, want_dist=want_dist, nwant=int((want >= 0).sum()), ref_inner=ref_inner, ref_whole=ref_whole)


@pytest.mark.parametrize("L,pa,pb", LISTS)
@pytest.mark.parametrize("n1", N1)
def test_shared_scan_at_its_edges(n1, L, pa, pb):
    c = _case(n1, L, pa, pb)
    k1, d1, k2, d2, z1, z2, F12, ex, ey, sf, sg = (c[k] for k in ("k1", "d1", "k2", "d2", "z1", "z2", "F12", "ex", "ey", "sf", "sg"))
    # the oracle against the construction
    r12, rbd = c["ref_inner"]
    assert np.array_equal(r12, c["want"]) and np.array_equal(rbd, c["want_dist"])
    assert (c["want_dist"] <= ORBmatcher.TH_LOW).all()
    for ori in (False, True):
        w12, wn = c["ref_whole"][ori]
        assert wn == c["nwant"] == (n1 if L else 0) and np.array_equal(w12, c["want"])
    # explicit CSR lists
    g12, gbd = ORBmatcher(0.6, False).match_triangulation(k1, d1, k2, d2, c["off"], c["idx"], z1, z2, z1, z2, F12, ex, ey, sf, sg, bOnlyStereo=False)
    assert np.array_equal(g12, r12) and np.array_equal(gbd, rbd)
    f1, f2 = Frame(k1, d1, (0.0, 0.0, 640.0, 480.0)), Frame(k2, d2, (0.0, 0.0, 640.0, 480.0))
    try:
        for ori in (False, True):
            w12, wn = c["ref_whole"][ori]
            m = ORBmatcher(0.6, ori)
            # the whole function on host arrays
            pairs, nm, m12 = m.SearchForTriangulation(k1, d1, c["fv1"], z1, z1, k2, d2, c["fv2"], z2, z2, F12, ex, ey, sf, sg, False)
            assert nm == wn and np.array_equal(m12, w12)
            assert np.array_equal(pairs[:, 0], np.nonzero(w12 >= 0)[0]) and np.array_equal(pairs[:, 1], w12[w12 >= 0])
            # ... and on two resident frames
            pairs, nm, m12 = m.frame_search_for_triangulation(f1, c["fv1"], z1, f2, c["fv2"], z2, F12, ex, ey, sf, sg, False)
            assert nm == wn and np.array_equal(m12, w12)
            assert np.array_equal(pairs[:, 0], np.nonzero(w12 >= 0)[0]) and np.array_equal(pairs[:, 1], w12[w12 >= 0])
    finally:
        f1.close(); f2.close()
