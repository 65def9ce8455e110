"""orbm_pnp_hypotheses on the device: every EPnP RANSAC hypothesis of PnPsolver in one call, and the host classes above it.

The acceptance rule is equality with the literal CPU restatement (tests/pnp_oracle.c) BIT FOR BIT: every field of every hypothesis
(the doubles as uint64 patterns), both mask arrays and the record flags.  The kernels instantiate orb_slam2_e_amd/csrc/orbm_epnp.h,
whose host instantiation tests/test_cpu_pnp.py holds to the same restatement; every step is + - * / sqrt on IEEE doubles with
-ffp-contract=off, so there is no tolerance to state.  One thing IEEE 754 leaves open is a NaN's sign and payload: an invalid
operation gives the negative quiet NaN on x86 and the positive one on gfx950, and which operand's NaN an operation passes on
differs as well.  A field that is NaN on one side must be NaN on the other; its sign and payload are not compared."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pnp_oracle as po
import pnp_scenes as scenes
import test_cpu_pnp as cpu
from orb_slam2_e_amd import _lib
from orb_slam2_e_amd import pnp

pytestmark = pytest.mark.gpu
SG = scenes.SIGMA2
FIELDS_F8, FIELDS_I4 = ("R", "t", "rep_error", "Rr", "tr"), ("ninliers", "refined", "nrefined", "pad")


def _c(p):
    return pnp.PnpProblem(p["Xw"], p["uv"], p["octave"], p["cam"], p["sets"], p["min_inliers"], p["th2"])


def _patterns(a, H):
    """the doubles as uint64 bit patterns, every NaN as the same one"""
    a = np.ascontiguousarray(a, np.float64).reshape(H, -1)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def _assert_equal(p, got, best_in=0):
    """one problem's device result against the restatement, bit for bit"""
    hyp, masks, rmasks = got
    assert len(hyp) == p["H"]
    if p["H"] == 0:
        return None
    o = po.hypotheses(p, SG, best_in)
    o["pad"] = np.zeros(p["H"], np.int32)
    for f in FIELDS_F8:
        a, b = _patterns(hyp[f], p["H"]), _patterns(o[f], p["H"])
        bad = np.flatnonzero((a != b).any(axis=1))
        assert len(bad) == 0, (p["name"], f, len(bad), bad[:5])
    for f in FIELDS_I4:
        assert (hyp[f] == o[f]).all(), (p["name"], f)
    if p["H"]:
        assert (masks == po.masks_of(o["flags"])).all() and (rmasks == po.masks_of(o["rflags"])).all(), p["name"]
        assert (rmasks[hyp["refined"] == 0] == 0).all()
    return o


def _degenerate_problem():
    """the degenerate sets of the CPU test inside a batch of ordinary ones"""
    q = scenes.problem(77, 30, 40, outliers=0.2)
    Xw, uv, octave, sets = scenes.degenerate_sets(q, np.random.default_rng(3))
    mixed = np.concatenate([q["sets"][:20], sets, q["sets"][20:]])
    return dict(q, name="degenerate", n=len(Xw), H=len(mixed), Xw=Xw, uv=uv, octave=octave, sets=mixed, min_inliers=8)


def _refine_problem(n):
    """all n correspondences are planted inliers: the first all-inlier set is a record whose Refine set has n members"""
    return scenes.problem(300 + n, n, 6, outliers=0.0, min_inliers=min(n, 8), name=f"refine{n}")


@pytest.mark.parametrize("n", [4, 63, 64, 65, 130])
@pytest.mark.parametrize("H", [1, 5, 64, 300])
def test_one_problem_equals_the_restatement(n, H):
    p = scenes.problem(1000 + 7 * n + H, n, H, outliers=0.25 if n > 4 else 0.0, min_inliers=4 if n == 4 else None)
    _assert_equal(p, pnp.pnp_hypotheses([_c(p)], SG)[0])
    assert pnp.last_pnp_waits() == 1


def test_three_problems_with_an_empty_one_between():
    probs = [scenes.problem(41, 65, 64), scenes.problem(42, 12, 0), scenes.problem(43, 130, 5)]
    res = pnp.pnp_hypotheses([_c(p) for p in probs], SG)
    assert pnp.last_pnp_waits() == 1 and len(res[1][0]) == 0
    for p, r in zip(probs, res):
        _assert_equal(p, r)


def test_sixty_four_small_problems():
    probs = [scenes.problem(500 + k, 20, 8, outliers=0.2) for k in range(64)]
    for p, r in zip(probs, pnp.pnp_hypotheses([_c(p) for p in probs], SG)):
        _assert_equal(p, r)


def test_degenerate_sets_inside_a_batch():
    p = _degenerate_problem()
    o = _assert_equal(p, pnp.pnp_hypotheses([_c(p)], SG)[0])
    assert o["singular"][21] > 0                                    # four times the same correspondence: qr_solve's early return
    assert not np.isfinite(o["R"][26]).all() and o["ninliers"][26] == 0    # a NaN coordinate: a NaN pose, never an inlier


def test_best_in_above_and_below_every_count():
    p = scenes.fold_scenes()[0]
    top = int(po.hypotheses(p, SG)["ninliers"].max())
    above = pnp.pnp_hypotheses([_c(p)], SG, [top])[0]
    assert above[0]["refined"].sum() == 0 and (above[2] == 0).all()          # no record: no Refine, the refined masks stay 0
    _assert_equal(p, above, top)
    below = pnp.pnp_hypotheses([_c(p)], SG, [-5])[0]
    assert below[0]["refined"].sum() >= 2
    _assert_equal(p, below, -5)
    both = pnp.pnp_hypotheses([_c(p), _c(p)], SG, [top, 0])                  # best_in is per problem
    _assert_equal(p, both[0], top); _assert_equal(p, both[1], 0)


@pytest.mark.parametrize("n", [4, 64, 65, 130])
def test_refine_set_sizes(n):
    p = _refine_problem(n)
    got = pnp.pnp_hypotheses([_c(p)], SG)[0]
    o = _assert_equal(p, got)
    rec = np.flatnonzero(got[0]["refined"])
    full = [k for k in rec if got[0]["ninliers"][k] == n]
    assert full, (n, o["ninliers"])                                  # a Refine set of exactly n members ran
    assert got[0]["nrefined"][full[0]] == n


def test_same_bytes_alone_first_last_and_twice():
    p, a, b = scenes.problem(61, 65, 40), scenes.problem(62, 130, 30), scenes.problem(63, 20, 50)
    alone = pnp.pnp_hypotheses([_c(p)], SG)[0]
    again = pnp.pnp_hypotheses([_c(p)], SG)[0]
    first = pnp.pnp_hypotheses([_c(p), _c(a), _c(b)], SG)[0]
    last = pnp.pnp_hypotheses([_c(a), _c(b), _c(p)], SG)[2]
    for other in (again, first, last):
        for x, y in zip(alone, other):
            assert x.tobytes() == y.tobytes()


def test_sentinels_around_every_output_array():
    probs = [scenes.problem(71, 65, 9), scenes.problem(72, 130, 5)]
    cs = [_c(p) for p in probs]
    arr = (pnp._CPnpProblem * 2)(*[c.c() for c in cs])
    total = sum(p["H"] for p in probs); words = sum(p["H"] * ((p["n"] + 63) // 64) for p in probs)
    pad = 4
    hyp = np.zeros(total + 2 * pad, pnp.HYPOTHESIS_DTYPE); hyp.view(np.uint8)[:] = 0xA5
    masks = np.full(words + 2 * pad, 0xA5A5A5A5A5A5A5A5, np.uint64); rmasks = masks.copy()
    L = _lib.lib()
    rc = L.orbm_pnp_hypotheses(arr, 2, _lib.ptr(SG), len(SG), None, hyp[pad:].ctypes.data, masks[pad:].ctypes.data, rmasks[pad:].ctypes.data)
    assert rc == 0 and L.orbm_debug_last_pnp_waits() == 1
    for a in (hyp.view(np.uint8).reshape(len(hyp), -1), masks.view(np.uint8).reshape(len(masks), -1), rmasks.view(np.uint8).reshape(len(rmasks), -1)):
        assert (a[:pad] == 0xA5).all() and (a[-pad:] == 0xA5).all()
    h0 = w0 = 0
    for p in probs:
        W = (p["n"] + 63) // 64
        _assert_equal(p, (hyp[pad + h0:pad + h0 + p["H"]], masks[pad + w0:pad + w0 + p["H"] * W].reshape(p["H"], W),
                          rmasks[pad + w0:pad + w0 + p["H"] * W].reshape(p["H"], W)))
        h0 += p["H"]; w0 += p["H"] * W


def test_nothing_to_do_is_no_launch():
    pnp.pnp_hypotheses([_c(scenes.problem(1, 20, 3))], SG)
    assert pnp.last_pnp_waits() == 1
    assert pnp.pnp_hypotheses([], SG) == [] and pnp.last_pnp_waits() == 0
    pnp.pnp_hypotheses([_c(scenes.problem(1, 20, 0))], SG)
    assert pnp.last_pnp_waits() == 0


# ------------------------------------------------------------------------------------------------ the classes above it
PARAMS = ((8, 300), (60, 12), (12, 300))          # (minInliers, maxIterations) per fold scene


def _fold_scene(k):
    p = scenes.fold_scenes()[k]
    return dict(p, sets=scenes.draw_sets(np.random.default_rng(5 + k), p["n"], 1024))


@pytest.mark.parametrize("calls", [[300], [5, 5, 5, 5], [1, 400, 3]])
def test_python_class_returns_the_restatement_fold(calls):
    for k, (min_in, max_its) in enumerate(PARAMS):
        p = _fold_scene(k)
        idx = np.arange(p["n"]) * 2 + 1
        s = pnp.PnPsolver(p["Xw"], p["uv"], p["octave"], p["cam"], SG, sets=p["sets"], indices=idx, n_matches=2 * p["n"] + 3)
        s.SetRansacParameters(0.99, min_in, max_its)
        o = po.Solver(p, SG, minInliers=min_in, maxIterations=max_its)
        for n in calls:
            T, no_more, inl, nin = s.iterate(n)
            To, no_more_o, flags_o, nin_o, _h, _kind = o.iterate(n)
            assert (T is None) == (To is None) and no_more == no_more_o and nin == nin_o, (p["name"], n)
            assert (s.mnIterations, s.mnBestInliers) == (o.fold.iterations, o.fold.best_inliers)
            if T is not None:
                assert T.tobytes() == To.tobytes() and (np.flatnonzero(inl) == idx[flags_o]).all()


def test_two_solvers_together_return_what_each_returns_alone():
    a, b = _fold_scene(0), _fold_scene(2)
    mk = lambda p: pnp.PnPsolver(p["Xw"], p["uv"], p["octave"], p["cam"], SG, sets=p["sets"])
    sa, sb = mk(a), mk(b)
    pnp.PnPsolver.evaluate([sa, sb])
    assert pnp.last_pnp_waits() == 1
    for s, q in ((sa, a), (sb, b)):
        ra = s.find()
        assert pnp.last_pnp_waits() == 1                                   # a fold, no device work
        rb = mk(q).find()
        assert ra[0].tobytes() == rb[0].tobytes() and (ra[1] == rb[1]).all() and ra[2] == rb[2]
        assert (ra[1] == q["inlier"]).all()                                 # the planted inlier set


def test_cxx_class_returns_the_restatement_fold(tmp_path):
    """tests/cxx/pnp_smoke.cpp: three solvers evaluated in one call, then each solver's iterate calls against the restatement's fold"""
    exe = cpu.build_smoke(tmp_path)
    calls = [5, 5, 300]
    files = []
    for k, (min_in, max_its) in enumerate(PARAMS):
        files.append(str(tmp_path / f"scene{k}.txt"))
        cpu.write_scene(files[-1], _fold_scene(k), min_in, max_its, calls, stride=2, extra=3)
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK 3 solvers in one call"), out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("call ")]
    assert len(lines) == 3 * len(calls)
    it = iter(lines)
    for k, (min_in, max_its) in enumerate(PARAMS):
        p = _fold_scene(k)
        o = po.Solver(p, SG, minInliers=min_in, maxIterations=max_its)
        for n in calls:
            head, tail = next(it).split(":")
            w = head.split()
            To, no_more_o, flags_o, nin_o, _h, _kind = o.iterate(n)
            assert int(w[1]) == k and bool(int(w[2])) == (To is not None) and bool(int(w[3])) == no_more_o and int(w[4]) == nin_o, (k, n, head)
            places = [int(v) for v in tail.split()]
            if To is not None:
                assert [int(v, 16) for v in w[5:21]] == To.reshape(16).view(np.uint32).tolist()
                assert places == (2 * np.flatnonzero(flags_o)).tolist()
            else:
                assert places == []
