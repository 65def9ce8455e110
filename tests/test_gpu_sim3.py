"""orbm_sim3_hypotheses on the device: every RANSAC hypothesis of Sim3Solver in one launch, and the host class above it.

* sizes at the wave and mask-word edges, ragged batches, the same bits alone / in a batch / from run to run, one host wait;
* planted degenerates against the CPU restatement (tests/sim3_oracle.c) and against their known answers;
* the scenes of the cap check against the restatement: hypotheses that agree bit for bit must have equal masks and counts; the
  others are counted (at most 2 %) and their flags compared where the restatement's gap is at least M;
* Sim3Solver.iterate / find against the restatement's fold, call by call.
"""
import random

import numpy as np
import pytest

import sim3_oracle as so
import sim3_scenes as scenes
from orb_slam2_e_amd import Sim3Problem, Sim3Solver, sim3_hypotheses
from orb_slam2_e_amd.sim3 import last_sim3_waits

pytestmark = pytest.mark.gpu

SG = scenes.SIGMA2

# Device against restatement over scenes.restatement_scenes() (1,350 hypotheses): the number of hypotheses whose T12 / R12 / t12 /
# s12 differ in any bit, and D = the largest relative difference of a differing hypothesis' T12, max |T12_device - T12_restatement|
# over its entries divided by the largest |entry| of the restatement's T12.  The rule (the project's,
# tests/test_gpu_create_points.py): D <= 1e-3 / 8, and the flags of a differing hypothesis are compared where the restatement's gap
# is at least M = 8 D.  With no differing hypothesis D = 0 and every flag is compared.
# MEASURED_D is the figure of one run on an MI355X; None = not measured yet (no MI355X could be had when this file was written): the
# tests then take the D of their own run, held to the same 1e-3 / 8, and print it for whoever pins it here.
MEASURED_DIFFERING = None
MEASURED_D = None
D_MAX = 1e-3 / 8
CAP = 0.02


def dev_problem(p, triples=None, H=None):
    tri = p["triples"] if triples is None else triples
    if H is not None:
        tri = tri[:H]
    return Sim3Problem(p["X1w"], p["X2w"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"], tri, p["fix_scale"])


def same_bits(a, b):
    """equal bit for bit; a NaN equals a NaN (the payload of a NaN is the processor's, not the arithmetic's)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def differing(hyp, ref):
    """[H] bool: the hypothesis differs from the restatement's in any bit of T12, R12, t12, s12"""
    eq = same_bits(hyp["T12"], ref["T12"]).all(1) & same_bits(hyp["R12"], ref["R12"]).all(1) & same_bits(hyp["t12"], ref["t12"]).all(1) \
        & same_bits(hyp["s12"], ref["s12"])
    return ~eq


def unpack(masks, n):
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(len(masks), -1), axis=1, bitorder="little")[:, :n].astype(bool)


def check_against_restatement(p, hyp, masks, ref=None):
    """the rule of the module docstring on one problem; returns (number of differing hypotheses, their largest relative T12 difference)"""
    n, H = p["n"], len(hyp)
    ref = ref or so.hypotheses(dict(p, H=H, triples=np.asarray(p["triples"])[:H]), SG)
    flags = unpack(masks, n)
    assert np.array_equal(masks, so.masks_of(flags)), "bits past n must be 0"
    assert np.array_equal(hyp["ninliers"], flags.sum(1)), "the count is the popcount of the mask"
    diff = differing(hyp, ref)
    same = ~diff
    assert np.array_equal(flags[same], ref["flags"][same]) and np.array_equal(hyp["ninliers"][same], ref["ninliers"][same]), p.get("name")
    D = 0.0
    for h in np.nonzero(diff)[0]:
        a, b = hyp["T12"][h].astype(np.float64), ref["T12"][h].astype(np.float64)
        d = np.abs(a - b)
        d[np.isnan(a) & np.isnan(b)] = 0.0
        d[np.isnan(d)] = np.inf                             # a NaN on one side only
        D = max(D, float(d.max() / np.nanmax(np.abs(b)))) if np.isfinite(b).any() else max(D, float(d.max()))
    assert D <= D_MAX, (p.get("name"), D)
    M = 8 * (D if MEASURED_D is None else MEASURED_D)
    for h in np.nonzero(diff)[0]:
        far = ref["gap"][h] >= M
        assert np.array_equal(flags[h][far], ref["flags"][h][far]), (p.get("name"), h)
    return int(diff.sum()), D


# ------------------------------------------------------------------------------------------------ sizes, batching, determinism
@pytest.fixture(scope="module")
def edge_problems():
    """n at the wave and mask-word edges x H in {1, 5, 300}, each run alone once"""
    out = []
    for k, n in enumerate((3, 4, 63, 64, 65, 129)):
        for H in (1, 5, 300):
            p = scenes.problem(100 + k, n, H, noise=1.0, outliers=0.3 if n > 4 else 0.0, name=f"edge_n{n}_H{H}")
            (hyp, masks), = sim3_hypotheses([dev_problem(p)], SG)
            assert last_sim3_waits() == 1
            out.append((p, hyp.copy(), masks.copy()))
    return out


def test_sizes_at_the_wave_and_mask_word_edges(edge_problems):
    total = ndiff = 0
    for p, hyp, masks in edge_problems:
        assert hyp.shape == (p["H"],) and masks.shape == (p["H"], (p["n"] + 63) // 64)
        d, D = check_against_restatement(p, hyp, masks)
        assert D <= D_MAX
        ndiff += d; total += p["H"]
    print("edge problems:", total, "hypotheses,", ndiff, "differ from the restatement in some bit")
    assert ndiff <= CAP * total


def test_a_problem_gives_the_same_bits_alone_and_in_a_ragged_batch(edge_problems):
    by = {p["name"]: (p, hyp, masks) for p, hyp, masks in edge_problems}
    for names in (("edge_n65_H5", "edge_n3_H1", "edge_n129_H300"), ("edge_n64_H300", "edge_n4_H5", "edge_n63_H1")):
        got = sim3_hypotheses([dev_problem(by[k][0]) for k in names], SG)
        assert last_sim3_waits() == 1
        for k, (hyp, masks) in zip(names, got):
            assert hyp.tobytes() == by[k][1].tobytes() and masks.tobytes() == by[k][2].tobytes(), k
    # a problem without hypotheses between two others takes no part
    a, b = by["edge_n65_H300"], by["edge_n129_H5"]
    got = sim3_hypotheses([dev_problem(a[0]), dev_problem(a[0], H=0), dev_problem(b[0])], SG)
    assert got[0][0].tobytes() == a[1].tobytes() and got[0][1].tobytes() == a[2].tobytes()
    assert got[1][0].shape == (0,) and got[2][0].tobytes() == b[1].tobytes() and got[2][1].tobytes() == b[2].tobytes()


def test_the_same_bits_from_run_to_run_and_the_wait_count(edge_problems):
    p, hyp, masks = next(e for e in edge_problems if e[0]["name"] == "edge_n129_H300")
    for _ in range(2):
        (h2, m2), = sim3_hypotheses([dev_problem(p)], SG)
        assert h2.tobytes() == hyp.tobytes() and m2.tobytes() == masks.tobytes()
        assert last_sim3_waits() == 1
    assert sim3_hypotheses([], SG) == [] and last_sim3_waits() == 0
    sim3_hypotheses([dev_problem(p)], SG)
    got = sim3_hypotheses([dev_problem(p, H=0), dev_problem(p, H=0)], SG)           # every H == 0: nothing is launched
    assert last_sim3_waits() == 0 and all(h.shape == (0,) for h, _ in got)


# ------------------------------------------------------------------------------------------------ planted degenerates
def planted():
    """Both poses are the identity, so the camera-frame points are the given floats.  20 exact correspondences of the similarity
    (s, R, t) of the scenes, then the planted ones; triple 0 is a good one."""
    I = np.eye(4, dtype=np.float32)
    p = scenes.problem(7, 20, 1)
    R, t, s = p["R"], p["t"], p["s"]
    to2 = lambda X1: ((np.asarray(X1, np.float64) - t) @ R / s)
    rng = np.random.default_rng(5)
    z = rng.uniform(2, 8, 20)
    X1 = np.stack([rng.uniform(-0.5, 0.5, 20) * z, rng.uniform(-0.4, 0.4, 20) * z, z], 1)
    names = {}
    extra1, extra2 = [], []

    def add(name, x1, x2=None):
        names[name] = 20 + len(extra1)
        extra1.append(np.asarray(x1, np.float64)); extra2.append(to2(x1) if x2 is None else np.asarray(x2, np.float64))

    line = np.array([0.5, -0.25, 4.0]); step = np.array([0.25, 0.5, 0.125])
    for k in range(3):
        add(f"line{k}", line + k * step)                       # three collinear points (exact in float)
    add("twin_a", [1.0, 0.5, 5.0]); add("twin_b", [1.0, 0.5, 5.0])   # two coincident points
    add("z_zero", [0.5, 0.25, 0.0])                            # camera-frame z = 0 in keyframe 1
    add("z_negative", [0.5, -0.75, -3.0])                      # behind camera 1, consistent with the similarity
    add("nan", [np.nan, 1.0, 4.0], [0.1, 0.2, 3.0])
    X1 = np.concatenate([X1, np.array(extra1)]); X2 = np.concatenate([to2(X1[:20]), np.array(extra2)])
    n = len(X1)
    tri = np.array([[0, 7, 13],
                    [names["line0"], names["line1"], names["line2"]],
                    [names["twin_a"], names["twin_b"], 3],
                    [1, names["nan"], 2],
                    [names["z_negative"], 5, 9]], np.int32)
    q = dict(p, n=n, H=len(tri), X1w=X1.astype(np.float32), X2w=X2.astype(np.float32), octave1=np.full(n, 2, np.int32),
             octave2=np.full(n, 3, np.int32), Tcw1=I, Tcw2=I, triples=tri, name="planted")
    return q, names


def test_planted_degenerates():
    q, names = planted()
    (hyp, masks), = sim3_hypotheses([dev_problem(q)], SG)
    ref = so.hypotheses(q, SG)
    d, D = check_against_restatement(q, hyp, masks, ref)
    assert D <= D_MAX
    flags = unpack(masks, q["n"])
    # the good triple: the similarity, every exact correspondence in, and no depth test: z < 0 is in, z = 0 and NaN are out
    assert np.allclose(hyp["R12"][0].reshape(3, 3), q["R"], atol=1e-4) and abs(hyp["s12"][0] - q["s"]) < 1e-4 * q["s"]
    assert flags[0, :20].all() and flags[0, names["z_negative"]] and flags[0, names["twin_a"]] and flags[0, names["line1"]]
    assert not flags[0, names["z_zero"]] and not flags[0, names["nan"]]
    assert not flags[:, names["nan"]].any() and not flags[:, names["z_zero"]].any()
    # a triple through the point behind the camera is a triple like any other
    assert flags[4, :20].all() and abs(hyp["s12"][4] - q["s"]) < 1e-4 * q["s"]
    # a NaN in the triple: NaN throughout, no inlier
    assert np.isnan(hyp["R12"][3]).all() and hyp["ninliers"][3] == 0
    assert np.isnan(ref["R12"][3]).all()
    # the collinear and the coincident triple have no known answer (the rotation about the line is not determined): they are held
    # to the restatement by check_against_restatement above, like every other hypothesis


def test_the_exact_identity_gives_nan_and_no_inlier():
    """P1 == P2 exactly: the leading eigenvector is (+-1, 0, 0, 0), norm(vec) = 0 and :280 is 0 / 0 -- NaN throughout, as in the
    reference; the known answer is 'no inliers'"""
    p = scenes.problem(9, 30, 5)
    q = dict(p, X2w=p["X1w"], Tcw2=p["Tcw1"], cam2=p["cam1"], name="identity")
    (hyp, masks), = sim3_hypotheses([dev_problem(q)], SG)
    ref = so.hypotheses(q, SG)
    assert np.isnan(hyp["T12"][:, :12]).all() and np.isnan(ref["T12"][:, :12]).all()
    assert (hyp["ninliers"] == 0).all() and not masks.any() and (ref["ninliers"] == 0).all()
    assert np.array_equal(hyp["T12"][:, 12:], np.tile(np.float32([0, 0, 0, 1]), (5, 1)))


# ------------------------------------------------------------------------------------------------ the scenes of the cap check
def test_scenes_against_the_restatement():
    total = ndiff = 0
    D = 0.0
    probs = scenes.restatement_scenes()
    got = sim3_hypotheses([dev_problem(p) for p in probs], SG)
    for p, (hyp, masks) in zip(probs, got):
        d, Dp = check_against_restatement(p, hyp, masks)
        print(p["name"], "hypotheses", len(hyp), "differing", d, "largest relative T12 difference", Dp, "best count", int(hyp["ninliers"].max()))
        ndiff += d; total += len(hyp); D = max(D, Dp)
    print("all scenes:", total, "hypotheses,", ndiff, "differing, D =", D)
    assert ndiff <= CAP * total
    assert D <= D_MAX
    if MEASURED_D is not None:
        assert D <= MEASURED_D and ndiff <= MEASURED_DIFFERING      # the figures M was derived from still hold


# ------------------------------------------------------------------------------------------------ the host class
def _candidates():
    return [scenes.problem(21, 120, 0, noise=1.0, outliers=0.4, name="cand0"), scenes.problem(22, 60, 0, noise=1.5, outliers=0.3, name="cand1"),
            scenes.problem(23, 200, 0, noise=1.0, outliers=0.5, fix_scale=True, name="cand2")]


def _solver(p, seed, **kw):
    return Sim3Solver(p["X1w"], p["X2w"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"], SG, p["fix_scale"],
                      draw=random.Random(seed).randint, **kw)


def test_iterate_round_robin_equals_the_restatement_call_by_call():
    cands = _candidates()
    mins = (20, 12, 30)
    dev = [_solver(p, 40 + k) for k, p in enumerate(cands)]
    ref = [so.Solver(p, SG, randint=random.Random(40 + k).randint) for k, p in enumerate(cands)]
    for s, r, m in zip(dev, ref, mins):
        s.SetRansacParameters(0.99, m, 300); r.SetRansacParameters(0.99, m, 300)
        assert s.mRansacMaxIts == r.fold.max_its
    Sim3Solver.EvaluateBatch(dev)
    assert last_sim3_waits() == 1                                   # three candidates, one launch
    for s, r, p in zip(dev, ref, cands):                            # the restatement runs the same triples
        r._evaluate()
        assert np.array_equal(r.prob["triples"], s.triples)
        d, D = check_against_restatement(dict(p, triples=r.prob["triples"]), s._hyp, s._masks, r.hyp)
        assert D <= D_MAX
    successes = [0, 0, 0]
    live = [True, True, True]
    calls = 0
    while any(live):
        for k, (s, r) in enumerate(zip(dev, ref)):
            if not live[k]:
                continue
            T, no_more, inl, nin = s.iterate(5)
            h, r_no_more, r_inl, r_nin = r.iterate(5)
            calls += 1
            assert no_more == r_no_more and nin == r_nin and (T is None) == (h < 0), (k, calls)
            assert s.mnIterations == r.fold.iterations and s.mnBestInliers == r.fold.best_inliers
            if T is not None:
                successes[k] += 1
                assert same_bits(T.reshape(16), r.hyp["T12"][h]).all() and np.array_equal(inl, r_inl)
                assert same_bits(s.GetEstimatedRotation().reshape(9), r.hyp["R12"][h]).all()
                assert same_bits(s.GetEstimatedTranslation().reshape(3), r.hyp["t12"][h]).all()
                assert np.float32(s.GetEstimatedScale()) == r.hyp["s12"][h] and nin > s.mRansacMinInliers
            else:
                assert not inl.any() and nin == 0
            live[k] = not no_more
    assert last_sim3_waits() == 1                                   # no device work after the first evaluation
    print("iterate(5) round-robin:", calls, "calls, successes per candidate", successes)
    assert max(successes) >= 2                                      # a candidate that succeeds twice


def test_find_equals_iterate_of_all_iterations():
    p = _candidates()[0]
    a, b = _solver(p, 77), _solver(p, 77)
    Ta, inl_a, na = a.find()
    Tb, no_more, inl_b, nb = b.iterate(b.mRansacMaxIts)
    assert (Ta is None) == (Tb is None) and na == nb and np.array_equal(inl_a, inl_b)
    assert Ta is not None and same_bits(Ta.reshape(16), Tb.reshape(16)).all() and a.mnIterations == b.mnIterations
    # vbInliers has the shape of vpMatched12: pairs kept at every second place of a vector twice as long
    c = _solver(p, 77, indices1=2 * np.arange(p["n"]), N1=2 * p["n"])
    Tc, inl_c, nc = c.find()
    assert nc == na and np.array_equal(inl_c[::2], inl_a) and not inl_c[1::2].any()
    # fewer pairs than minInliers: at once, without a launch
    few = scenes.problem(3, 5, 0)
    sim3_hypotheses([], SG)
    T, no_more, inl, n = _solver(few, 1).iterate(5)
    assert T is None and no_more and n == 0 and last_sim3_waits() == 0
