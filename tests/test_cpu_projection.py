"""The projection prefix of the SearchByProjection family on the CPU: the numpy restatement (tests/projection_reference.py)
against the C oracle (oracle/match_oracle.c) bit for bit on the edge scenes of tests/projection_scenes.py and on the synthetic
tracking scenes; every boundary pair lies on its boundary (its two entries, one ulp apart, have different outcomes); known
answers by construction.  No GPU."""
import numpy as np
import pytest

import oracle
import projection_reference as R
import projection_scenes as S
from orb_slam2_e_amd.synth import synth_tracking_scene

f32 = np.float32


def same(a, b, what=""):
    """Structured or plain arrays equal: floats as bits, except that two NaNs are equal whatever their payloads."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    for f in (a.dtype.names or [None]):
        x, y = (a[f], b[f]) if f else (a, b)
        if x.dtype.kind == "f":
            nx, ny = np.isnan(x), np.isnan(y)
            assert np.array_equal(nx, ny), (what, f, np.flatnonzero(nx != ny))
            k = ~nx
            bad = np.flatnonzero(x[k].view(np.uint32) != y[k].view(np.uint32))
            assert not len(bad), (what, f, np.flatnonzero(k)[bad], x[k][bad], y[k][bad])
        else:
            assert np.array_equal(x, y), (what, f, np.flatnonzero(x != y))


def restate_pp(sc, bounds=None):
    return R.project_points(sc["mode"], sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["Rcw"], sc["tcw"], sc["Ow"], sc["cam"],
                            bounds or sc["bounds"], sc["mbf"], sc["cos_limit"], sc["ls"], sc["sf"], sc["th"])


def oracle_pp(sc, bounds=None):
    return oracle.project_points(sc["mode"], sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["Rcw"], sc["tcw"], sc["Ow"], sc["cam"],
                                 np.array(bounds or sc["bounds"], f32), sc["mbf"], sc["cos_limit"], sc["ls"], sc["sf"], sc["th"])


FRUSTUM = [(m, p, th) for m in (0, 1, 2) for p in ("ref", "fork") for th in (1.0, float(np.nextafter(f32(1), f32(2))))]


@pytest.mark.parametrize("mode,pyr,th", FRUSTUM)
def test_project_points_restatement_equals_the_oracle(mode, pyr, th):
    sc = S.frustum_scene(mode, pyr, th)
    out, q, code, clamp = restate_pp(sc)
    oo, oq = oracle_pp(sc)
    same(out, oo, "projected"); same(q, oq, "queries")
    assert np.array_equal(out["visible"] == 1, code >= R.ACCEPTED)
    variants, _ = S.project_bounds_variants(sc)
    for name, b in variants:
        same(restate_pp(sc, b)[1], oracle_pp(sc, b)[1], name)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_project_points_minus_zero(mode):
    sc = S.minus_zero_scene(mode)
    Rc = R.gemm(sc["Rcw"], sc["pos"][1], sc["tcw"])
    assert Rc[2] == 0 and np.signbit(Rc[2])
    out, q, code, _ = restate_pp(sc)
    oo, oq = oracle_pp(sc)
    same(out, oo); same(q, oq)


@pytest.mark.parametrize("mode,pyr", [(m, p) for m in (0, 1, 2) for p in ("ref", "fork")])
def test_boundary_pairs_sit_on_their_boundary(mode, pyr):
    """The two entries of every pair differ by one ulp in one input and in outcome (code, level or radius)."""
    sc = S.frustum_scene(mode, pyr)
    out, q, code, _ = restate_pp(sc)
    for i, j, name in sc["pairs"]:
        a = (code[i], out["level"][i], q["r"].view(np.uint32)[i]); b = (code[j], out["level"][j], q["r"].view(np.uint32)[j])
        assert a != b, name
        diff = [k for k in ("mind", "maxd") if sc[k][i] != sc[k][j]] + [k for k in range(3) if sc["nrm"][i][k] != sc["nrm"][j][k]]
        assert len(diff) == 1, name
    names = {n for _, _, n in sc["pairs"]}
    assert {"near", "far", f"level{len(sc['sf']) - 1}"} <= names
    assert ({"cos_limit", "radius", "radius_offaxis"} if mode == 0 else {"dot_half"}) <= names


def test_known_answers():
    """By construction: on the axis viewCos is the normal's z; the 0.998 pair straddles the double constant (one side 3.0, the other
    4.5); a ratio of +inf (maxd = inf, a point at the camera centre) takes level 0 as x86-64's conversion makes it; the fork's
    pyramid clamps a point at 1.2 maxd to level 0 from below."""
    for pyr in ("ref", "fork"):
        sc = S.frustum_scene(0, pyr)
        out, q, code, clamp = restate_pp(sc)
        t = np.array(sc["tag"])
        i, j = [p[:2] for p in sc["pairs"] if p[2] == "radius"][0]
        assert out["view_cos"][i] == sc["nrm"][i][2] and out["view_cos"][j] == sc["nrm"][j][2]
        assert float(out["view_cos"][i]) <= 0.998 < float(out["view_cos"][j])
        assert (code[i], code[j]) == (R.ACCEPTED_WIDE, R.ACCEPTED)
        assert q["r"][i] == f32(4.5) * sc["sf"][out["level"][i]] and q["r"][j] == f32(3.0) * sc["sf"][out["level"][j]]
        for k in np.flatnonzero((t == "maxd_inf") | (t == "centre")):
            assert code[k] >= R.ACCEPTED and out["level"][k] == 0 and clamp[k] == R.LEVEL_LOW, sc["tag"][k]
        k = np.flatnonzero(t == "maxd_huge")[0]                            # a finite ratio of 2e38: the top level
        assert out["level"][k] == len(sc["sf"]) - 1 and clamp[k] == R.LEVEL_HIGH
        assert (code[t == "pos_nan"] >= R.ACCEPTED).all() and np.isnan(out["u"][t == "pos_nan"]).all()
        k = np.flatnonzero(t == "z_pos0")[0]
        assert code[k] == R.ACCEPTED and np.isnan(out["u"][k])       # 0 * inf: NaN passes the bounds test
        assert code[np.flatnonzero(t == "z_pos0_inf")[0]] == R.OUT_U
        for m in (1, 2):
            s2 = S.frustum_scene(m, pyr)
            c2 = restate_pp(s2)
            k = s2["tag"].index("level_low")
            assert c2[2][k] == R.ACCEPTED and c2[3][k] == (R.LEVEL_LOW if pyr == "fork" else R.LEVEL_IN)
            assert c2[2][s2["tag"].index("z_pos0")] == R.OUT_U                # IsInImage refuses NaN


def _forms(sc, th_kf=None):
    """(restated, oracle) queries of LAST, KF, SIM3 and both PAIR directions on a form scene or a synthetic tracking scene."""
    mono = not sc.get("stereo", False)
    res = {}
    v = sc["valid"]
    q, c, _ = R.form_last(sc["Tcw"], sc["Tlw"], v, sc["pos"], sc["octave"], sc["cam"], sc["bounds"], sc["sf"], sc["mb"], sc["mbf"],
                          sc["th"], mono)
    o = oracle.search_by_projection_last(sc["kps"], sc["desc"], sc["uright"], sc["occupied"], sc["bounds"], sc["cam"], sc["mb"], sc["mbf"],
                                         sc["Tcw"], sc["sf"], sc["Tlw"], v, sc["pos"], sc["mp_desc"], np.ones(len(v), np.uint8),
                                         sc["octave"], sc["angle"], sc["th"], mono)
    res["last"] = (q, c, o[3])
    q, c, cl = R.form_kf(sc["Tcw"], v, sc["pos"], sc["mind"], sc["maxd"], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], sc["th"])
    o = oracle.search_by_projection_kf(sc["kps"], sc["desc"], sc["occupied"], sc["bounds"], sc["cam"], sc["Tcw"], sc["sf"], sc["ls"], v,
                                       sc["pos"], sc["mind"], sc["maxd"], sc["mp_desc"], sc["angle"], sc["th"], 100)
    res["kf"] = (q, c, o[3], cl)
    th3 = int(sc["th"])
    q, c, cl = R.form_sim3(sc["Scw"], v, sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], th3)
    o = oracle.search_by_projection_sim3(sc["kps"], sc["desc"], sc["occupied"], sc["bounds"], sc["cam"], sc["Scw"], sc["sf"], sc["ls"], v,
                                         sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["mp_desc"], th3)
    res["sim3"] = (q, c, o[3], cl)
    take = np.arange(len(sc["kps2"])) % len(v)        # key frame 2's points: the same entries again, one per keypoint
    a, b = R.form_pair(sc["Tcw"], sc["T2w"], sc["s12"], sc["R12"], sc["t12"], v, sc["pos"], sc["mind"], sc["maxd"], v[take],
                       sc["pos"][take], sc["mind"][take], sc["maxd"][take], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], sc["th"])
    o = oracle.search_by_sim3_whole(_fit_kps(sc["kps"], len(v)), _fit_desc(sc["desc"], len(v)), sc["kps2"], sc["desc2"], sc["bounds"], sc["cam"], sc["sf"], sc["ls"],
                                    sc["Tcw"], sc["T2w"], sc["s12"], sc["R12"], sc["t12"], v, sc["pos"], sc["mind"], sc["maxd"],
                                    sc["mp_desc"], v[take], sc["pos"][take], sc["mind"][take], sc["maxd"][take], sc["mp_desc"][take],
                                    sc["th"])
    res["pair12"] = (a[0], a[1], o[4], a[2]); res["pair21"] = (b[0], b[1], o[5], b[2])
    return res


def _fit_kps(k, n):
    """Key frame 1 of SearchBySim3 has one keypoint per entry: the frame's first n keypoints, repeated if it has fewer."""
    return np.ascontiguousarray(k[np.arange(n) % len(k)])


def _fit_desc(d, n):
    return np.ascontiguousarray(d[np.arange(n) % len(d)])


def tracking_as_form_scene(seed, stereo=False, motion="none"):
    s = synth_tracking_scene(seed, stereo=stereo, motion=motion)
    lm = s["last_mp"]
    n = len(lm)
    pos = s["pos"][lm]
    return dict(kps=s["kps"], desc=s["desc"], uright=s["uright"], occupied=s["occupied"], bounds=s["bounds"], cam=s["cam"], mb=s["mb"],
                mbf=s["mbf"], Tcw=s["Tcw"], Tlw=s["Tlw"], Scw=s["Scw"], T2w=s["T2w"], s12=s["s12"], R12=s["R12"], t12=s["t12"],
                sf=s["scale_factors"], ls=s["log_scale_factor"], valid=s["last_valid"], pos=pos, octave=s["last_octave"],
                angle=s["last_angle"], mp_desc=s["mp_desc"][lm], mind=s["mind"][lm], maxd=s["maxd"][lm], nrm=s["normal"][lm],
                th=f32(7.0), kps2=s["kps2"], desc2=s["desc2"], stereo=stereo, motion=motion, n=n)


FORM_SCENES = [("edges", 1, "ref", False, "none"), ("edges", 2, "fork", True, "forward"), ("edges", 3, "ref", True, "backward"),
               ("edges", 4, "fork", False, "none"), ("synthetic", 11, None, False, "none"), ("synthetic", 13, None, True, "forward")]


def form_scene(kind, seed, pyr, stereo, motion):
    return S.form_scene(seed, pyr, stereo, motion) if kind == "edges" else tracking_as_form_scene(seed, stereo, motion)


@pytest.mark.parametrize("kind,seed,pyr,stereo,motion", FORM_SCENES)
def test_form_queries_equal_the_oracle(kind, seed, pyr, stereo, motion):
    sc = form_scene(kind, seed, pyr, stereo, motion)
    for name, (q, code, oq, *_) in _forms(sc).items():
        same(q, oq, name)
        assert np.array_equal(q["r"] >= 0, code == R.ACCEPTED), name


def test_form_outcomes_reached():
    """Across the edge scenes every outcome each form can reach occurs, and the clamps both ways."""
    seen = {}
    for kind, seed, pyr, stereo, motion in FORM_SCENES[:4]:
        for name, (q, code, oq, *cl) in _forms(form_scene(kind, seed, pyr, stereo, motion)).items():
            seen.setdefault(name, set()).update(code.tolist())
            if cl:
                seen.setdefault(name + "_clamp", set()).update(cl[0][cl[0] >= 0].tolist())
    A = set(range(R.ACCEPTED + 1))
    assert seen["last"] == {R.INVALID, R.BEHIND, R.OUT_U, R.OUT_V, R.ACCEPTED}, seen["last"]
    assert seen["kf"] == A - {R.BEHIND, R.VIEW_ANGLE}, seen["kf"]
    assert seen["sim3"] == A, seen["sim3"]
    assert seen["pair12"] == A - {R.VIEW_ANGLE}, seen["pair12"]
    for f in ("kf", "sim3", "pair12"):
        assert seen[f + "_clamp"] == {R.LEVEL_IN, R.LEVEL_LOW, R.LEVEL_HIGH}, (f, seen[f + "_clamp"])


def test_three_maxima_at_the_ten_percent_rule():
    for h in S.histogram_cases():
        assert R.three_maxima(h) == oracle.three_maxima(h), h[h > 0]
    h = S.histogram_cases()[0]                      # max1 = 30, max2 = 3: 0.1f * 30 rounds to 3.0f exactly, so 3 < 3 fails: bin 17 stays
    assert R.three_maxima(h) == (3, 17, -1)
    h = S.histogram_cases()[7]                      # 3 of 31: 3 < 3.1f, dropped (an integer max1 / 10 would keep it)
    assert R.three_maxima(h) == (3, -1, -1)
    h = S.histogram_cases()[2]                      # 4 and 3 of 30: both stay
    assert R.three_maxima(h) == (3, 17, 8)


def test_rotation_bins_at_their_edges():
    """rot * (1/30) at k + 0.5 rounds away from zero; one ulp below it rounds down; the wrap: rot just below 0 becomes 360 - tiny,
    bin 12 (round(360 / 30)); bin 30 never occurs, so its wrap to 0 is dead code."""
    bins = [R.rot_bin(a, b) for a, b in S.rotation_angles()]
    fac = f32(f32(1) / f32(30))
    for k in range(12):
        t, lo, hi = bins[3 * k:3 * k + 3]
        x = f32(f32(f32(k + 0.5) / fac) * fac)
        assert t == (k + 1 if x >= f32(k + 0.5) else k) and lo <= t <= hi and hi == k + 1 and lo in (k, k + 1)
    assert set(bins) <= set(range(13)) and 12 in bins


def test_window_restatement_equals_the_oracle():
    """GetFeaturesInArea with the level range, strict |dx| < r / |dy| < r and the stereo test, against oracle.search_window on the
    lattice scene: the best of query i is its target keypoint exactly when the restatement lists it as a candidate."""
    w = S.window_scene()
    k = w["kps"]
    g = R.Grid(k["x"], k["y"], w["bounds"])
    best, bl, second, sl, idx = oracle.search_window(w["queries"], w["qdesc"], k, w["desc"], w["bounds"], None, w["uright"])
    reasons = {}
    for i, q in enumerate(w["queries"]):
        c = g.window(q["u"], q["v"], q["r"], int(q["min_level"]), int(q["max_level"]), k["octave"], None, w["uright"], q["xr"])
        t = int(w["target"][i])
        rs = [r for j, r in c if j == t]
        cand = [j for j, r in c if r == R.W_IN]
        assert (idx[i] == t) == (t in cand), (i, w["tags"][i], q, rs)
        assert idx[i] in cand or idx[i] == -1
        reasons.setdefault(w["tags"][i], set()).update(rs)
    assert reasons["dx"] == {R.W_IN, R.W_DX} and reasons["dy"] == {R.W_IN, R.W_DY}
    assert reasons["level"] == {R.W_IN, R.W_LEVEL} and reasons["uright"] == {R.W_IN, R.W_URIGHT}


def test_nan_keypoints_leave_the_grid():
    """PosInGrid of a NaN coordinate: (int)roundf(NaN) is INT_MIN on x86-64, so the keypoint is outside the grid (the reference
    never returns it from a window); +-inf and 1e10 leave it too."""
    kps, _ = S.nan_keypoints()
    g = R.Grid(kps["x"], kps["y"], S.BOUNDS)
    fin = np.isfinite(kps["x"]) & np.isfinite(kps["y"]) & (np.abs(kps["x"]) < 1e9) & (np.abs(kps["y"]) < 1e9)
    assert (g.cell[~fin] < 0).all()
    inner = fin & (kps["x"] < 630) & (kps["y"] < 470)
    assert (g.cell[inner] >= 0).all()
    assert R.f2i(f32(np.nan)) == R.f2i(f32(np.inf)) == R.f2i(f32(-np.inf)) == R.f2i(f32(2.0 ** 31)) == R.INT_MIN
    assert R.f2i(f32(-2.0 ** 31)) == R.INT_MIN and R.f2i(f32(2.0 ** 31 - 128)) == 2 ** 31 - 128 and R.f2i(f32(-2.5)) == -2


@pytest.mark.parametrize("counts", S.ROTATION_COUNTS + [None], ids=[str(c) for c in S.ROTATION_COUNTS] + ["bin_edges"])
def test_rotation_check_equals_the_oracle(counts):
    """The whole rotation check (bin of every match, ComputeThreeMaxima, removal) on matches known by construction: the oracle's
    literal loop clears exactly the matches the restated rule drops."""
    sc = S.rotation_scene(counts)
    bins, kept = S.rotation_kept(sc)
    mk, mq, nm = oracle.search_projection_seq(sc["queries"], sc["qdesc"], sc["qangle"], sc["takes"], sc["kps"], sc["desc"], sc["bounds"])
    n = len(bins)
    assert np.array_equal(mq, np.arange(n)) and nm == kept.sum()
    assert np.array_equal(mk, np.where(kept, np.arange(n), -2))
    if counts == {0: 31, 5: 3, 9: 2}:               # 3 < 0.1f * 31: only bin 0 stays
        assert set(bins[kept]) == {0}
    if counts == {0: 30, 5: 3, 9: 2}:               # 3 < 0.1f * 30 = 3.0f fails: bins 0 and 5 stay
        assert set(bins[kept]) == {0, 5}
