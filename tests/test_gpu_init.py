"""orbm_init_find_models / orbm_init_check_rt / orbm_init_reconstruct_f on the device: every H / F hypothesis of a monocular
initialisation in one launch, up to 8 CheckRT passes in one more, and the host classes above them.

* sizes at the minimum set and at the wave and mask-word edges, the same bytes from run to run, one host wait (none when nothing
  launches), the reported winners = the first strict maximum of the device's own scores;
* the scenes against the CPU restatement (tests/init_oracle.c): a hypothesis whose matrix and score equal the restatement's bit for
  bit must have an equal mask; the others are counted (at most 2 %), the largest relative difference D of their matrices must be at
  most 1e-3 / 8, and their flags are compared where both of the restatement's chiSquares lie outside [th / 2, 2 th];
* planted quirks through the device; CheckRT per motion; Initializer.initialize against the restatement's Initialize; the C++ class.

Why the band suffices: a relative matrix error of 1.25e-4 moves a projected point of a 640 x 480 scene by under about 0.3 px; the
threshold distance at sigma = 1 is 2.45 px (H) and the band edges are at 1.73 and 3.46 px.
"""
import os
import subprocess

import numpy as np
import pytest

import init_oracle as io
import init_scenes as scenes
from orb_slam2_e_amd import Initializer, check_rt, find_models, last_init_waits, reconstruct_f
from orb_slam2_e_amd import initializer as ini

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_e_amd")
K = scenes.K

# Device against restatement over scenes.compared_scenes(): the number of (model, hypothesis) pairs whose matrix or score differ in
# any bit, and D = the largest relative difference of a differing matrix (max entry difference over the largest entry of the
# restatement's).  MEASURED_D is the figure of one run on an MI355X; None = not pinned yet: the tests then take the D of their own
# run, held to the same 1e-3 / 8, and print it for whoever pins it here.  (The run this file was written against: 0 of 3,672
# hypotheses differing, D = 0; left unpinned, since 0 would turn the first last-bit difference of the device's hypot into a failure.)
MEASURED_DIFFERING = None
MEASURED_D = None
D_MAX = 1e-3 / 8
CAP = 0.02
TH = (io.TH_H, io.TH_F)


def same_bits(a, b):
    """equal bit for bit; a NaN equals a NaN (the payload of a NaN is the processor's, not the arithmetic's)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def rel_diff(a, b):
    """max |a - b| over max |b|; NaN on both sides agrees, on one side only is infinite"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    d[np.isnan(a) & np.isnan(b)] = 0.0
    d[np.isnan(d)] = np.inf
    scale = np.nanmax(np.abs(b)) if np.isfinite(b).any() else 1.0
    return float(d.max() / scale) if scale > 0 else float(d.max())


def run(s, **kw):
    return find_models(s["keys1"], s["keys2"], s["matches"], s["sets"], s.get("sigma", 1.0), per_hypothesis=True, **kw)


def ref_of(s):
    return io.find_models(s["keys1"], s["keys2"], s["matches"], s["sets"], s.get("sigma", 1.0))


def check_own_fold(s, d):
    """independent of any difference: the winners are the first strict maxima of the device's OWN scores, starting from 0; their
    matrices and masks are those hypotheses'; bits past n are 0"""
    n, H = s["n"], len(s["sets"])
    flags = ini.unpack_mask(d["masks"], n)
    assert np.array_equal(d["masks"], io.masks_of(flags)), "bits past n must be 0"
    for model, (M, S, it, mask) in enumerate(((d["H21"], d["SH"], d["itH"], d["maskH"]), (d["F21"], d["SF"], d["itF"], d["maskF"]))):
        best, want = np.float32(0), -1
        for h in range(H):
            if d["scores"][model, h] > best:
                best, want = d["scores"][model, h], h
        assert it == want and same_bits(S, best).all(), (s["name"], model)
        if want >= 0:
            assert same_bits(M, d["matrices"][model, want]).all() and np.array_equal(mask, d["masks"][model, want])
        else:
            assert not M.any() and not mask.any() and S == 0
    return flags


def check_against_restatement(s, d, r=None):
    """the rule of the module docstring on one scene; returns (differing hypotheses, their largest relative matrix difference)"""
    r = r or ref_of(s)
    flags = check_own_fold(s, d)
    H = len(s["sets"])
    same = same_bits(d["matrices"].reshape(2, H, 9), r["matrices"].reshape(2, H, 9)).all(2) & same_bits(d["scores"], r["scores"])
    assert np.array_equal(flags[same], r["flags"][same]), s["name"]
    D = 0.0
    for model, h in np.argwhere(~same):
        D = max(D, rel_diff(d["matrices"][model, h], r["matrices"][model, h]))
    assert D <= D_MAX, (s["name"], D)
    for model, h in np.argwhere(~same):
        c, th = r["chi"][model, h], TH[model]
        far = ~(((c >= th / 2) & (c <= 2 * th)).any(1))
        assert np.array_equal(flags[model, h][far], r["flags"][model, h][far]), (s["name"], model, h)
    if same.all():                                              # then the folds agree too
        assert (d["itH"], d["itF"]) == (r["itH"], r["itF"]) and same_bits(d["SH"], r["SH"]).all() and same_bits(d["SF"], r["SF"]).all()
        assert np.array_equal(d["inliersH"], r["inliersH"]) and np.array_equal(d["inliersF"], r["inliersF"])
    return int((~same).sum()), D


# ------------------------------------------------------------------------------------------------ sizes, determinism, the rule
@pytest.fixture(scope="module")
def edge_runs():
    out = []
    for s in scenes.edge_scenes():
        d = run(s)
        assert last_init_waits() == 1
        out.append((s, d))
    return out


def test_sizes_at_the_minimum_set_and_the_wave_and_mask_word_edges(edge_runs):
    assert sorted({s["n"] for s, _ in edge_runs}) == [8, 9, 63, 64, 65, 129] and sorted({s["H"] for s, _ in edge_runs}) == [1, 5, 200]
    total = ndiff = 0
    D = 0.0
    for s, d in edge_runs:
        assert d["matrices"].shape == (2, s["H"], 3, 3) and d["masks"].shape == (2, s["H"], (s["n"] + 63) // 64)
        k, Ds = check_against_restatement(s, d)
        ndiff += k; total += 2 * s["H"]; D = max(D, Ds)
    print("edge scenes:", total, "hypotheses,", ndiff, "differ from the restatement in some bit, D =", D)
    assert ndiff <= CAP * total and D <= D_MAX


def test_the_same_bytes_from_run_to_run_and_the_wait_count(edge_runs):
    s, d = next(e for e in edge_runs if e[0]["name"] == "edge_n129_H200")
    for _ in range(2):
        d2 = run(s)
        assert last_init_waits() == 1
        for key in ("matrices", "scores", "masks", "H21", "F21", "maskH", "maskF"):
            assert np.asarray(d2[key]).tobytes() == np.asarray(d[key]).tobytes(), key
    none = find_models(s["keys1"], s["keys2"], s["matches"], np.zeros((0, 8), np.int32))        # H == 0: nothing is launched
    assert last_init_waits() == 0 and (none["itH"], none["itF"], none["SH"], none["SF"]) == (-1, -1, 0, 0) and not none["inliersH"].any()
    plain = find_models(s["keys1"], s["keys2"], s["matches"], s["sets"])                        # without the per-hypothesis arrays
    assert last_init_waits() == 1 and plain["H21"].tobytes() == d["H21"].tobytes() and plain["maskF"].tobytes() == d["maskF"].tobytes()


def test_scenes_against_the_restatement():
    total = ndiff = 0
    D = 0.0
    for s in scenes.restatement_scenes():
        d = run(s)
        k, Ds = check_against_restatement(s, d)
        print(s["name"], "hypotheses", 2 * s["H"], "differing", k, "largest relative matrix difference", Ds, "SH", d["SH"], "SF", d["SF"])
        ndiff += k; total += 2 * s["H"]; D = max(D, Ds)
    print("all scenes:", total, "hypotheses,", ndiff, "differing, D =", D)
    assert ndiff <= CAP * total and D <= D_MAX
    if MEASURED_D is not None:
        assert D <= MEASURED_D and ndiff <= MEASURED_DIFFERING


# ------------------------------------------------------------------------------------------------ planted quirks
def test_a_singular_homography_scores_nan_and_never_wins():
    s = scenes.singular_scene()
    d, r = run(s), ref_of(s)
    check_against_restatement(s, d, r)
    assert np.isnan(d["scores"][0, 0]) and np.isnan(r["scores"][0, 0])
    assert np.count_nonzero(d["matrices"][0, 0]) <= 3 and ini.unpack_mask(d["masks"][0, 0], s["n"]).all()
    assert d["itH"] >= 1 and d["SH"] > 0
    alone = find_models(s["keys1"], s["keys2"], s["matches"], s["sets"][:1], per_hypothesis=True)
    assert np.isnan(alone["scores"][0, 0])
    assert (alone["itH"], alone["SH"]) == (-1, 0) and not alone["inliersH"].any() and alone["inliersH"].shape == (48,) and not alone["H21"].any()


def test_a_score_of_zero_never_wins_and_both_models_can_lose():
    s = scenes.zero_score_scene()
    d = run(s)
    check_against_restatement(s, d)
    assert ((d["scores"] == 0) | np.isnan(d["scores"])).all() and (d["scores"][1] == 0).sum() > 0
    assert (d["itH"], d["itF"], d["SH"], d["SF"]) == (-1, -1, 0, 0) and not d["maskH"].any() and not d["maskF"].any() and not d["F21"].any()
    init = Initializer(s["keys1"], K, s["sigma"], len(s["sets"]))
    st, R21, t21, P3D, tri = init.initialize(s["keys2"], s["matches12"], sets=s["sets"])
    assert st == ini.NO_FUNDAMENTAL and np.isnan(init.RH) and not tri.any() and not P3D.any()


# ------------------------------------------------------------------------------------------------ CheckRT
def _motions(s, M):
    """the truth and the other three of its decomposition, then the four again under a further rotation of 2 degrees"""
    tx = np.array([[0, -s["t"][2], s["t"][1]], [s["t"][2], 0, -s["t"][0]], [-s["t"][1], s["t"][0], 0]])
    R1, R2, t = io.decompose_e((tx @ s["R"]).astype(np.float32))
    Rs, ts = [R1, R2, R1, R2], [t, t, -t, -t]
    dR = scenes.rotation((0.3, -1.0, 0.2), 2.0).astype(np.float32)
    Rs += [(dR @ R).astype(np.float32) for R in Rs]; ts += ts
    order = [k for k in range(8) if np.abs(Rs[k] - s["R"]).max() < 1e-3 and ts[k] @ s["t"] > 0] + list(range(8))
    pick = list(dict.fromkeys(order))[:M]                     # the true motion first
    return np.stack([Rs[k] for k in pick]), np.stack([ts[k] for k in pick])


def check_rt_against_restatement(s, d, inl, R, t, th2):
    """orbm_init_check_rt's result d for the motions (R[m], t[m]) against the restatement, motion by motion: bit for bit where the
    triangulated points agree bit for bit, otherwise the counted flags away from the thresholds and the points within D_MAX"""
    n = len(s["matches"])
    for m in range(len(R)):
        r = io.check_rt(s["keys1"], s["keys2"], s["matches"], inl, K, R[m], t[m], th2)
        assert not d["counted"][m][~inl].any() and d["ngood"][m] == d["counted"][m].sum()
        if same_bits(d["P3D"][m], r["P3D"]).all() and same_bits(d["cos_parallax"][m], r["cos_parallax"]).all():
            assert d["ngood"][m] == r["ngood"] and np.array_equal(d["good"][m], r["good"]) and np.array_equal(d["counted"][m], r["counted"])
            assert same_bits(d["parallax"][m], r["parallax"]).all(), (n, m)
        else:
            far = ~(((r["err"] >= th2 / 2) & (r["err"] <= 2 * th2)).any(1)) & (r["err"] >= 0).all(1)
            assert np.array_equal(d["counted"][m][far], r["counted"][far]), (n, m)
            both = d["counted"][m] & r["counted"]
            first = s["matches"][both, 0]
            assert rel_diff(d["P3D"][m][first], r["P3D"][first]) <= D_MAX, (n, m)


def rt_scene(n, M):
    """(scene, inlier flags with some outliers on and some inliers off, M motions: the true one first)"""
    s = scenes.scene(400 + n, n, 1, "general", noise=0.3, outliers=0.1, name=f"rt_n{n}")
    inl = ~s["bad"]; inl[::7] = ~inl[::7]
    return (s, inl) + _motions(s, M)


@pytest.mark.parametrize("M", [1, 4, 8])
def test_check_rt_against_the_restatement(M):
    th2 = np.float32(4.0)
    for n in (8, 9, 63, 64, 65, 129):
        s, inl, R, t = rt_scene(n, M)
        d = check_rt(s["keys1"], s["keys2"], s["matches"], inl, K, R, t, th2)
        assert last_init_waits() == 1 and d["good"].shape == (M, len(s["keys1"])) and d["counted"].shape == (M, n)
        check_rt_against_restatement(s, d, inl, R, t, th2)
        assert d["ngood"][0] >= 0.7 * inl.sum()                 # the true motion triangulates the inliers
    # the decision edges of the CPU file through the device
    k1, k2, mt, R, t, X = scenes.rt_scene([4.0, 5.0, 3000.0, -4.0, -3000.0])
    d = check_rt(k1, k2, mt, np.ones(5), K, np.tile(R, (M, 1, 1)), np.tile(t, (M, 1)), 4.0)
    r = io.check_rt(k1, k2, mt, np.ones(5), K, R, t, 4.0)
    for m in range(M):
        assert d["counted"][m].tolist() == [True, True, True, False, True] and d["good"][m][:5].tolist() == [True, True, False, False, False]
        assert d["P3D"][m][2].any() and not d["P3D"][m][3].any() and d["ngood"][m] == r["ngood"] == 4
    none = check_rt(k1, k2, mt, np.zeros(5), K, np.tile(R, (M, 1, 1)), np.tile(t, (M, 1)), 4.0)
    assert not none["ngood"].any() and not none["parallax"].any() and not none["P3D"].any()
    check_rt(k1, k2, mt, np.ones(5), K, np.zeros((0, 3, 3)), np.zeros((0, 3)), 4.0)
    assert last_init_waits() == 0                               # M == 0: nothing is launched


@pytest.mark.parametrize("count", [1, 50, 51, 52])
def test_parallax_index_through_the_device(count):
    k1, k2, m, R, t, X = scenes.rt_scene(np.linspace(2.0, 12.0, count), t=(0.3, 0.0, 0.0))
    d = check_rt(k1, k2, m, np.ones(count), K, R[None], t[None], 4.0)
    r = io.check_rt(k1, k2, m, np.ones(count), K, R, t, 4.0)
    assert d["ngood"][0] == r["ngood"] == count
    if same_bits(d["cos_parallax"][0], r["cos_parallax"]).all():
        assert same_bits(d["parallax"][0], r["parallax"]).all()
    else:
        assert abs(d["parallax"][0] - r["parallax"]) <= 1e-4 * r["parallax"]


# ------------------------------------------------------------------------------------------------ the host classes
def _compare_initialize(s, H=200):
    init = Initializer(s["keys1"], K, 1.0, H)
    st, R21, t21, P3D, tri = init.initialize(s["keys2"], s["matches12"], sets=s["sets"])
    r = io.initialize(s["keys1"], s["keys2"], s["matches12"], s["sets"], K)
    assert np.array_equal(init.mvMatches12, r["matches"])
    ref = ref_of(s)
    exact = same_bits(init.models["F21"], ref["F21"]).all() and same_bits(init.models["SF"], ref["SF"]).all() \
        and same_bits(init.models["SH"], ref["SH"]).all() and np.array_equal(init.models["inliersF"], ref["inliersF"])
    if exact:
        assert st == r["status"] and same_bits(init.RH, r["RH"]).all()
        assert same_bits(R21, r["R21"]).all() and same_bits(t21, r["t21"]).all() and np.array_equal(tri, r["triangulated"])
        assert same_bits(P3D, r["P3D"]).all()
    else:
        assert st == r["status"] and rel_diff(R21, r["R21"]) <= D_MAX and rel_diff(t21, r["t21"]) <= D_MAX
        both = tri & r["triangulated"]
        assert both.sum() >= 0.98 * max(tri.sum(), r["triangulated"].sum()) and rel_diff(P3D[both], r["P3D"][both]) <= D_MAX
    return st, init, exact


def test_initializer_on_the_general_scene_against_the_restatement():
    s = scenes.scene(301, 300, 200, "general", scenes.NOISE, scenes.OUTLIERS)
    st, init, exact = _compare_initialize(s)
    print("general scene: status", st, "RH", init.RH, "models bit-equal to the restatement's:", bool(exact))
    assert st == ini.INITIALIZED and init.RH < 0.99
    assert np.abs(init.reconstruction["R21"] - s["R"]).max() < 5e-3
    assert last_init_waits() == 1
    # the draws through a callback, in the reference's order: the same sets from the same generator
    import random
    a = Initializer(s["keys1"], K, 1.0, 50); b = Initializer(s["keys1"], K, 1.0, 50)
    ra = a.initialize(s["keys2"], s["matches12"], draw=random.Random(5).randint)
    rb = b.initialize(s["keys2"], s["matches12"], sets=ini.draw_sets(s["n"], 50, random.Random(5).randint))
    assert np.array_equal(a.mvSets, b.mvSets) and ra[0] == rb[0] and all(np.array_equal(x, y) for x, y in zip(ra[1:], rb[1:]))


def test_the_planar_scene_with_rh_forced_above_0_99_wants_reconstruct_h(monkeypatch):
    """No data makes this fork's RH exceed 0.99 reliably (a fundamental matrix fits coplanar points as well as the homography does:
    RH is about 0.5), so SF is forced down between the launch and the ratio"""
    s = scenes.scene(302, 300, 200, "planar", scenes.NOISE, scenes.OUTLIERS)
    st, init, _ = _compare_initialize(s)
    assert st != ini.WANTS_RECONSTRUCT_H and 0.3 < init.RH < 0.7
    real = ini.find_models

    def forced(*a, **kw):
        out = real(*a, **kw)
        out["SF"] = np.float32(out["SF"] / 200)
        return out

    monkeypatch.setattr(ini, "find_models", forced)
    init = Initializer(s["keys1"], K, 1.0, 200)
    st, R21, t21, P3D, tri = init.initialize(s["keys2"], s["matches12"], sets=s["sets"])
    assert st == ini.WANTS_RECONSTRUCT_H and init.RH > 0.99 and init.reconstruction is None and not tri.any()
    assert init.models["itH"] >= 0 and init.models["inliersH"].sum() > 0.8 * s["n"]          # what the caller's ReconstructH is handed


def test_reconstruct_f_against_the_restatement():
    s = scenes.scene(301, 300, 200, "general", scenes.NOISE, scenes.OUTLIERS)
    ref = ref_of(s)
    for kw in (dict(), dict(min_triangulated=400), dict(min_parallax=90.0)):
        d = reconstruct_f(s["keys1"], s["keys2"], s["matches"], ref["inliersF"], ref["F21"], K, **kw)
        r = io.reconstruct_f(s["keys1"], s["keys2"], s["matches"], ref["inliersF"], ref["F21"], K, **kw)
        assert last_init_waits() == 1
        assert d["found"] == r["found"] and d["best"] == r["best"]
        if same_bits(d["P3D"], r["P3D"]).all():
            assert np.array_equal(d["ngood"], r["ngood"]) and same_bits(d["parallax"], r["parallax"]).all()
            assert same_bits(d["R21"], r["R21"]).all() and same_bits(d["t21"], r["t21"]).all() and np.array_equal(d["triangulated"], r["triangulated"])
        else:
            assert np.abs(d["ngood"] - r["ngood"]).max() <= CAP * s["n"] and rel_diff(d["R21"], r["R21"]) <= D_MAX
    assert reconstruct_f(s["keys1"], s["keys2"], s["matches"], ref["inliersF"], ref["F21"], K)["found"]


def test_cxx_class_on_the_device(tmp_path):
    exe = str(tmp_path / "init_smoke")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "init_smoke.cpp"),
                           "-o", exe, "-L", LIBDIR, "-lorbslam_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK initialised")
