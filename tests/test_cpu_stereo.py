"""Frame::ComputeStereoMatches (src/Frame.cc:527-701) on the CPU: the numpy restatement (tests/stereo_reference.py) against the C
oracle (oracle/stereo_oracle.c), known answers from geometry, the outcomes real images cannot reach, and the premise of the
stereo buffers' resize fix.  No GPU."""
import numpy as np
import pytest

import oracle
import stereo_reference as R
import stereo_scenes as S
from orb_slam2_e_amd.extractor import plan

f32 = np.float32
SCENES = {f.__name__ + (f"_{a}" if a is not None else ""): (f, a) for f, a in
          [(S.kitti03, None), (S.kitti04, None), (S.euroc_near_maxd, None), (S.fork_pyramid, None), (S.one_level, None),
           (S.coarse_pyramid, None), (S.shift, 0), (S.shift, 1), (S.shift, -8), (S.small_maxd, None), (S.photometric_right, None),
           (S.half_identical, None), (S.dense_band, None), (S.flat_left, None), (S.flat_right, None), (S.unrelated_noise, None),
           (S.tall, None)]}


def _both(sc, mb=None):
    oL, oR = oracle.OrbOracle(*sc["prm"]), oracle.OrbOracle(*sc["prm"])
    kL, dL = oL.extract(sc["left"]); kR, dR = oR.extract(sc["right"])
    mb = sc["mb"] if mb is None else f32(mb)
    ou, od, nd = oracle.stereo_matches(oL, oR, kL, dL, kR, dR, mb, sc["mbf"])
    return kL, kR, R.from_oracle(oL, oR, kL, dL, kR, dR, mb, sc["mbf"]), (ou, od, nd)


def _bits_equal(r, o):
    ou, od, nd = o
    return np.array_equal(r["uRight"].view(np.uint32), ou.view(np.uint32)) and np.array_equal(r["depth"].view(np.uint32), od.view(np.uint32)) \
        and r["nd"] == nd


@pytest.mark.parametrize("name", list(SCENES))
def test_restatement_equals_the_oracle(name):
    f, a = SCENES[name]
    sc = f(a) if a is not None else f()
    kL, kR, r, o = _both(sc)
    assert _bits_equal(r, o)
    assert np.all(r["code"] >= 0) and len(r["code"]) == len(kL)
    assert np.array_equal(r["uRight"] >= 0, np.isin(r["code"], (R.CLAMPED, R.ACCEPTED)))


def test_outcomes_the_scenes_reach():
    """The GPU module's scenes between them reach every outcome but two: BORDER and DELTA (see the tests below)."""
    seen = set()
    for f, a in SCENES.values():
        if f is S.tall:
            continue
        seen |= set(_both(f(a) if a is not None else f())[2]["code"].tolist())
    assert seen == set(range(9)) - {R.BORDER, R.DELTA}


@pytest.mark.parametrize("d", [1, 3, 17])
def test_integer_shift_known_answer(d):
    """right = left shifted by d: an accepted level-0 match on its shifted twin with a unique L1 minimum lies within half a pixel
    of uL - d, and depth = mbf / (uL - uR) in float."""
    sc = S.shift(d, seed=20 + d)
    kL, kR, r, o = _both(sc)
    assert _bits_equal(r, o)
    acc = r["code"] == R.ACCEPTED
    assert acc.sum() > 500
    br = r["best_right"]
    twin = acc & (kL["octave"] == 0) & r["unique_min"]
    twin &= (kR["octave"][br] == 0) & (kR["x"][br] == kL["x"] - d) & (kR["y"][br] == kL["y"])
    assert twin.sum() > 100
    assert np.all(np.abs(r["uRight"][twin] - (kL["x"][twin] - d)) <= 0.5)
    assert np.array_equal(r["depth"][acc].view(np.uint32), (sc["mbf"] / (kL["x"][acc] - r["uRight"][acc]).astype(f32)).astype(f32).view(np.uint32))


def test_identical_images_cut_every_match():
    """d = 0: the best L1 distance of every match is 0, so the median is 0, thDist is 0 and the cut takes every match."""
    kL, kR, r, o = _both(S.shift(0))
    assert _bits_equal(r, o) and r["nd"] > 500 and r["median"] == 0
    assert np.all(r["uRight"] == -1) and (r["code"] == R.MEDIAN_CUT).sum() == r["nd"]


def test_baseline_beyond_the_shift_accepts_nothing():
    """With maxD = mbf / mb = 4 px, far below the 20-px shift, the true twins lie outside [uL - maxD, uL]: nothing is accepted."""
    sc = S.shift(20, seed=30)
    kL, kR, r, o = _both(sc, mb=sc["mbf"] / f32(4.0))
    assert _bits_equal(r, o)
    assert not np.isin(r["code"], (R.ACCEPTED, R.CLAMPED)).any() and (r["uRight"] == -1).all()


def test_clamp_survives_the_median():
    kL, kR, r, o = _both(S.half_identical())
    assert _bits_equal(r, o) and r["median"] > 0
    cl = r["code"] == R.CLAMPED
    assert cl.sum() >= 5
    assert np.array_equal(r["uRight"][cl], (kL["x"][cl].astype(np.float64) - 0.01).astype(f32))
    assert np.all(r["depth"][cl] == S.half_identical()["mbf"] / f32(0.01))


def test_border_reject_with_hand_built_keypoints():
    """endu >= cols (:634-636).  Real keypoints lie at least 19 px inside their own level (FAST's border), so a right keypoint
    within 11 px of the right edge of the left keypoint's level needs a pyramid of scale near 2 and a match one octave down:
    the GPU scenes do not reach it.  Here hand-built keypoints go to the C oracle and to the restatement: the same pair is
    rejected with the right keypoint 10 px from the edge and matched 12 px from it."""
    sc = S.shift(0, seed=40)
    oL, oR = oracle.OrbOracle(*sc["prm"]), oracle.OrbOracle(*sc["prm"])
    kL, dL = oL.extract(sc["left"]); kR, dR = oR.extract(sc["right"])
    W = sc["left"].shape[1]
    k = np.zeros(1, oracle.KP_DTYPE); k["y"] = 240; k["octave"] = 0
    desc = dL[:1].copy()
    for gap, code in ((10, R.BORDER), (11, R.BORDER), (12, None)):
        kl = k.copy(); kl["x"] = W - gap + 4
        kr = k.copy(); kr["x"] = W - gap
        ou, od, nd = oracle.stereo_matches(oL, oR, kl, desc, kr, desc, sc["mb"], sc["mbf"])
        r = R.from_oracle(oL, oR, kl, desc, kr, desc, sc["mb"], sc["mbf"])
        assert _bits_equal(r, (ou, od, nd))
        if code is not None:
            assert r["code"][0] == code and ou[0] == -1
        else:
            assert r["code"][0] != R.BORDER


def test_delta_reject_cannot_happen():
    """|deltaR| > 1 (:666-669) is unreachable: d2 is the first minimum of the eleven distances, so d1 > d2 <= d3 and
    |d1 - d3| <= (d1 - d2) + (d3 - d2): |deltaR| <= 1/2.  Checked exhaustively in float32 over integer distances (the L1 norms
    are integers) up to 64 and on spread samples up to the largest 11 x 11 distance, 61,710."""
    a = np.arange(65, dtype=f32)
    d1, d2, d3 = np.meshgrid(a, a, a, indexing="ij")
    rng = np.random.default_rng(0)
    s = rng.integers(0, 61711, (3, 1 << 20)).astype(f32)
    for x1, x2, x3 in ((d1.ravel(), d2.ravel(), d3.ravel()), tuple(s)):
        m = (x1 > x2) & (x3 >= x2)
        x1, x2, x3 = x1[m], x2[m], x3[m]
        delta = (x1 - x3) / (f32(2.0) * ((x1 + x3) - f32(2.0) * x2))
        assert delta.dtype == f32 and np.all(np.abs(delta) <= 0.5)


def test_small_quota_capacity_follows_the_frame_size():
    """The premise of the stereo buffers' resize fix: a handle of 40 features holds 64 keypoints per frame at 640 x 480 and 128
    at 1242 x 375 (4 children of each of 4 initial octree nodes per level), so buffers sized at the first size are too small
    for the second."""
    a = plan(40, 1.2, 8, 20, 7, 640, 480)["keypoint_capacity"]
    b = plan(40, 1.2, 8, 20, 7, 1242, 375)["keypoint_capacity"]
    assert (a, b) == (64, 128)
