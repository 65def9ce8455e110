"""GPU: the projection prefix of the SearchByProjection family at its boundaries and degenerate points -- k_project_points
(modes 0 / 1 / 2), k_project_form (LAST / KF / SIM3 / PAIR through the whole searches), the window predicate of k_win_wave /
k_win_best and the grid layout of k_frame_build -- against the numpy restatement (tests/projection_reference.py) on the scenes of
tests/projection_scenes.py.  Window queries and projections are compared as float bits (two NaNs as NaN-ness only: x86 and the
GPU make different payloads), match arrays and counts as integers against the C oracle, under both resolvers.

The degenerate points are where the device used to differ from x86-64: PredictScale's level of a ratio of +inf (a point at the
camera centre with mfMinDistance 0, an infinite mfMaxDistance) and PosInGrid's cell of a NaN keypoint, both float -> int
conversions that C leaves undefined (orbx_f2i_x86 now gives them x86-64's meaning on the device).

Mutations that give the same output by construction: min_level >= 0 in check_levels (it differs from min_level > 0 only for a
window with levels [0, -1], where the added test, octave < 0, never holds) and the 10 % rule as 10 max2 < max1 in integers
(equal to the float rule for counts below about 10^6).

The last test checks that the scenes reached every outcome each form can reach.  Unreachable by construction: BEHIND in the KF
form (it has no depth test: :1706-1713) and VIEW_ANGLE in KF, LAST and PAIR (they have no viewing-angle test)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import projection_reference as R
import projection_scenes as S
from orb_slam2_e_amd import Frame, ORBmatcher, Points, View
from test_cpu_projection import FORM_SCENES, FRUSTUM, _fit_desc, _fit_kps, form_scene, restate_pp, same

SEEN = {}
f32 = np.float32


def _see(form, code, clamp=None):
    SEEN.setdefault(form, set()).update(code.tolist())
    if clamp is not None:
        SEEN.setdefault(form + "_clamp", set()).update(clamp[clamp >= 0].tolist())


def _device_pp(m, sc, bounds=None):
    """orbm_project_points: the bounds are the camera record's float grid bounds (mnMinX .. mnMaxY)."""
    b = np.array(bounds or sc["bounds"], np.float32)
    cam = np.zeros(1, m.CAM_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"] = S.CAM
    cam["gminx"], cam["gminy"], cam["gmaxx"], cam["gmaxy"] = b
    return m.project_points(sc["mode"], sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["Rcw"], sc["tcw"], sc["Ow"], cam, sc["mbf"],
                            sc["ls"], sc["sf"], float(sc["th"]), float(sc["cos_limit"]))


@pytest.mark.parametrize("mode,pyr,th", FRUSTUM)
def test_project_points_at_the_edges(mode, pyr, th):
    m = ORBmatcher(0.8, True)
    sc = S.frustum_scene(mode, pyr, th)
    out, q, code, clamp = restate_pp(sc)
    _see(f"mode{mode}", code, clamp)
    go, gq = _device_pp(m, sc)
    same(go, out, "projected"); same(gq, q, "queries")
    for i, j, name in sc["pairs"]:          # the device separates the two sides of every boundary as well
        assert (go["visible"][i], go["level"][i], gq["r"].view(np.uint32)[i]) != (go["visible"][j], go["level"][j],
                                                                                  gq["r"].view(np.uint32)[j]) or code[i] != code[j], name
    variants, k = S.project_bounds_variants(sc)
    vis = {}
    for name, b in variants:
        o, qq, c, _ = restate_pp(sc, b)
        go, gq = _device_pp(m, sc, b)
        same(go, o, name); same(gq, qq, name)
        vis[name] = int(c[k])
    # u = max_x passes isInFrustum's u > max_x and fails IsInImage's u < max_x; u = min_x passes both
    assert vis["max_x=u"] == (R.OUT_U if mode else vis["max_x=u+"]) and vis["max_x=u-"] == R.OUT_U and vis["max_x=u+"] >= R.ACCEPTED
    assert vis["min_x=u"] >= R.ACCEPTED and vis["min_x=u+"] == R.OUT_U
    assert vis["max_y=v"] == (R.OUT_V if mode else vis["max_y=v+"]) and vis["max_y=v-"] == R.OUT_V and vis["min_y=v+"] == R.OUT_V


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_project_points_minus_zero(mode):
    m = ORBmatcher(0.8, True)
    sc = S.minus_zero_scene(mode)
    out, q, code, _ = restate_pp(sc)
    go, gq = _device_pp(m, sc)
    same(go, out); same(gq, q)


def _view(sc):
    return View(*sc["cam"], float(sc["mb"]), float(sc["mbf"]), float(sc["ls"]), sc["sf"])


@pytest.mark.parametrize("kind,seed,pyr,stereo,motion", FORM_SCENES)
def test_whole_forms_at_the_edges(kind, seed, pyr, stereo, motion, resolver):
    """LAST, KF, SIM3 and SearchBySim3 on resident frames: queries against the restatement, matches against the oracle."""
    _check_forms(form_scene(kind, seed, pyr, stereo, motion))


@pytest.mark.parametrize("stereo", [False, True])
def test_whole_forms_with_bounds_on_a_projection(stereo):
    """The frame's bounds set to the u / v an entry projects to and one ulp either side: LAST and KF keep u = max_x (u > mnMaxX
    rejects), SIM3 and SearchBySim3 drop it (KeyFrame::IsInImage: u < mnMaxX); u = min_x passes all four."""
    sc = form_scene("edges", 5, "ref", stereo, "none")
    q, code, _ = R.form_kf(sc["Tcw"], sc["valid"], sc["pos"], sc["mind"], sc["maxd"], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], sc["th"])
    k = next(i for i, t in enumerate(sc["tag"]) if t == "aimed" and code[i] == R.ACCEPTED)
    u, v = f32(q["u"][k]), f32(q["v"][k])
    up, dn = lambda x: np.nextafter(x, f32(np.inf)), lambda x: np.nextafter(x, f32(-np.inf))
    b = [f32(x) for x in sc["bounds"]]
    codes = {}
    for name, bb in (("max_x=u", (b[0], b[1], u, b[3])), ("max_x=u-", (b[0], b[1], dn(u), b[3])), ("min_x=u", (u, b[1], b[2], b[3])),
                     ("min_x=u+", (up(u), b[1], b[2], b[3])), ("max_y=v", (b[0], b[1], b[2], v)), ("min_y=v+", (b[0], up(v), b[2], b[3]))):
        codes[name] = _check_forms(dict(sc, bounds=tuple(float(x) for x in bb)), k)
    assert codes["max_x=u"] == (R.ACCEPTED, R.ACCEPTED, R.OUT_U) and codes["max_y=v"] == (R.ACCEPTED, R.ACCEPTED, R.OUT_V)
    assert codes["max_x=u-"] == (R.OUT_U,) * 3 and codes["min_x=u+"] == (R.OUT_U,) * 3 and codes["min_y=v+"] == (R.OUT_V,) * 3
    assert codes["min_x=u"] == (R.ACCEPTED,) * 3


def _check_forms(sc, k=None):
    """The four whole searches on one scene; returns the restated (LAST, KF, SIM3) codes of entry k."""
    stereo = sc["stereo"]
    mono = not stereo
    mt = ORBmatcher(0.9, True)
    v = sc["valid"]
    n = len(v)
    cur = Frame(sc["kps"], sc["desc"], sc["bounds"], sc["uright"])
    takes = np.ones(n, np.uint8)
    # LAST
    rq, rc, _ = R.form_last(sc["Tcw"], sc["Tlw"], v, sc["pos"], sc["octave"], sc["cam"], sc["bounds"], sc["sf"], sc["mb"], sc["mbf"],
                            sc["th"], mono)
    _see("last", rc)
    ks = [rc[k] if k is not None else None]
    ref = oracle.search_by_projection_last(sc["kps"], sc["desc"], sc["uright"], sc["occupied"], sc["bounds"], sc["cam"], sc["mb"],
                                           sc["mbf"], sc["Tcw"], sc["sf"], sc["Tlw"], v, sc["pos"], sc["mp_desc"], takes, sc["octave"],
                                           sc["angle"], sc["th"], mono)
    last = Points(v, sc["pos"], sc["mp_desc"], takes=takes, octave=sc["octave"], angle=sc["angle"])
    got = mt.SearchByProjectionLast(cur, _view(sc), sc["Tcw"], sc["Tlw"], last, sc["occupied"], float(sc["th"]), mono, want_queries=True)
    same(got[3], rq, "last")
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    # KF
    rq, rc, cl = R.form_kf(sc["Tcw"], v, sc["pos"], sc["mind"], sc["maxd"], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], sc["th"])
    _see("kf", rc, cl)
    ks.append(rc[k] if k is not None else None)
    ref = oracle.search_by_projection_kf(sc["kps"], sc["desc"], sc["occupied"], sc["bounds"], sc["cam"], sc["Tcw"], sc["sf"], sc["ls"],
                                         v, sc["pos"], sc["mind"], sc["maxd"], sc["mp_desc"], sc["angle"], sc["th"], 100)
    kf = Points(v, sc["pos"], sc["mp_desc"], min_distance=sc["mind"], max_distance=sc["maxd"], angle=sc["angle"])
    got = mt.SearchByProjectionKeyFrame(cur, _view(sc), sc["Tcw"], kf, sc["occupied"], float(sc["th"]), 100, want_queries=True)
    same(got[3], rq, "kf")
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    cur.close()
    # SIM3 (a key frame: no right coordinates)
    th3 = int(sc["th"])
    rq, rc, cl = R.form_sim3(sc["Scw"], v, sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["cam"], sc["bounds"], sc["sf"], sc["ls"], th3)
    _see("sim3", rc, cl)
    ks.append(rc[k] if k is not None else None)
    ref = oracle.search_by_projection_sim3(sc["kps"], sc["desc"], sc["occupied"], sc["bounds"], sc["cam"], sc["Scw"], sc["sf"], sc["ls"],
                                           v, sc["pos"], sc["nrm"], sc["mind"], sc["maxd"], sc["mp_desc"], th3)
    kfr = Frame(sc["kps"], sc["desc"], sc["bounds"])
    pts = Points(v, sc["pos"], sc["mp_desc"], normal=sc["nrm"], min_distance=sc["mind"], max_distance=sc["maxd"])
    got = mt.SearchByProjectionSim3(kfr, _view(sc), sc["Scw"], pts, sc["occupied"], th3, want_queries=True)
    same(got[3], rq, "sim3")
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    kfr.close()
    # SearchBySim3: key frame 1 has one keypoint per entry, key frame 2's entries are the same points again
    take = np.arange(len(sc["kps2"])) % n
    k1, d1 = _fit_kps(sc["kps"], n), _fit_desc(sc["desc"], n)
    (q12, c12, l12), (q21, c21, l21) = R.form_pair(sc["Tcw"], sc["T2w"], sc["s12"], sc["R12"], sc["t12"], v, sc["pos"], sc["mind"],
                                                   sc["maxd"], v[take], sc["pos"][take], sc["mind"][take], sc["maxd"][take], sc["cam"],
                                                   sc["bounds"], sc["sf"], sc["ls"], sc["th"])
    _see("pair", c12, l12); _see("pair", c21, l21)
    ref = oracle.search_by_sim3_whole(k1, d1, sc["kps2"], sc["desc2"], sc["bounds"], sc["cam"], sc["sf"], sc["ls"], sc["Tcw"], sc["T2w"],
                                      sc["s12"], sc["R12"], sc["t12"], v, sc["pos"], sc["mind"], sc["maxd"], sc["mp_desc"], v[take],
                                      sc["pos"][take], sc["mind"][take], sc["maxd"][take], sc["mp_desc"][take], sc["th"])
    f1, f2 = Frame(k1, d1, sc["bounds"]), Frame(sc["kps2"], sc["desc2"], sc["bounds"])
    p1 = Points(v, sc["pos"], sc["mp_desc"], min_distance=sc["mind"], max_distance=sc["maxd"])
    p2 = Points(v[take], sc["pos"][take], sc["mp_desc"][take], min_distance=sc["mind"][take], max_distance=sc["maxd"][take])
    got = mt.SearchBySim3Whole(f1, f2, _view(sc), sc["Tcw"], sc["T2w"], sc["s12"], sc["R12"], sc["t12"], p1, p2, float(sc["th"]),
                               want_queries=True)
    same(got[4], q12, "q12"); same(got[5], q21, "q21")
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    f1.close(); f2.close()
    return tuple(ks)


def test_window_predicate_at_the_edges(resolver):
    """|dx| = r, |dy| = r and |xr - uright| = r exactly and one ulp either side, the level range's ends, r = 0 / < 0 / NaN, a NaN
    centre: the best of every query is its target keypoint exactly when the restatement lists the target as a candidate."""
    w = S.window_scene()
    k = w["kps"]
    g = R.Grid(k["x"], k["y"], w["bounds"])
    m = ORBmatcher(0.8, True)
    ref = oracle.search_window(w["queries"], w["qdesc"], k, w["desc"], w["bounds"], None, w["uright"])
    got = m.search_window(w["queries"], w["qdesc"], k, w["desc"], w["bounds"], None, w["uright"])
    f = Frame(k, w["desc"], w["bounds"], w["uright"])
    got2 = m.frame_search_window(f, w["queries"], w["qdesc"])
    f.close()
    for a, b, c in zip(got, got2, ref):
        assert np.array_equal(a, c) and np.array_equal(b, c)
    idx = got[4]
    for i, q in enumerate(w["queries"]):
        c = g.window(q["u"], q["v"], q["r"], int(q["min_level"]), int(q["max_level"]), k["octave"], None, w["uright"], q["xr"])
        t = int(w["target"][i])
        assert (idx[i] == t) == ((t, R.W_IN) in c), (i, w["tags"][i])


@pytest.mark.parametrize("counts", S.ROTATION_COUNTS + [None], ids=[str(c) for c in S.ROTATION_COUNTS] + ["bin_edges"])
def test_rotation_check_at_the_ten_percent_rule(counts, resolver):
    """Bins at ComputeThreeMaxima's 10 % rule (3 of 31 dropped, 3 of 30 kept) and angle differences on the bin edges and the
    360-degree wrap: the device clears exactly the matches the restated rule drops, host arrays and resident frame alike."""
    sc = S.rotation_scene(counts)
    bins, kept = S.rotation_kept(sc)
    n = len(bins)
    m = ORBmatcher(0.6, True)
    ref = oracle.search_projection_seq(sc["queries"], sc["qdesc"], sc["qangle"], sc["takes"], sc["kps"], sc["desc"], sc["bounds"])
    got = m.search_projection(sc["queries"], sc["qdesc"], sc["qangle"], sc["takes"], sc["kps"], sc["desc"], sc["bounds"], th_accept=95)
    f = Frame(sc["kps"], sc["desc"], sc["bounds"])
    got2 = m.frame_search_projection(f, sc["queries"], sc["qdesc"], sc["qangle"], sc["takes"], th_accept=95)
    f.close()
    for g in (got, got2):
        assert np.array_equal(g[0], ref[0]) and np.array_equal(g[1], ref[1]) and g[2] == ref[2]
        assert np.array_equal(g[0], np.where(kept, np.arange(n), -2)) and g[2] == kept.sum()


@pytest.mark.parametrize("case", ["nan_inf", "all_nan"])
def test_frame_layout_with_nan_keypoints(case):
    """k_frame_build against orbm_sorted_frame (the host sort) and the restated PosInGrid: NaN, +-inf and 1e10 coordinates leave
    the grid (x86-64: (int)roundf(NaN) = INT_MIN; the GPU's conversion would have put NaN in column / row 0)."""
    from orb_slam2_e_amd._lib import lib
    kps, desc = S.nan_keypoints()
    if case == "all_nan":
        kps["x"][:] = np.nan
    bounds = S.BOUNDS
    f = Frame(kps, desc, bounds)
    perm, cell_off = f.layout()
    L = lib()
    n = len(kps)
    rp = np.zeros(n, np.int32); rc = np.zeros(64 * 48 + 1, np.int32); ns = C.c_int(0)
    assert L.orbm_sorted_frame(kps.ctypes.data_as(C.c_void_p), n, None, None, *bounds, rp.ctypes.data_as(C.c_void_p),
                               rc.ctypes.data_as(C.c_void_p), C.byref(ns)) == 0
    gp, gc = R.Grid(kps["x"], kps["y"], bounds).layout()
    assert ns.value == len(gp) and np.array_equal(rp[:ns.value], gp) and np.array_equal(rc, gc)
    assert f.ns == len(gp) and np.array_equal(perm, gp) and np.array_equal(cell_off, gc)
    f.close()


def test_every_reachable_outcome_occurred():
    """Across this module (its tests run in file order) every outcome each form can reach occurred, and PredictScale clamped both
    ways in every form that calls it; the unreachable ones are listed in the module docstring."""
    A = set(range(R.ACCEPTED + 1))
    pp = A - {R.INVALID}                               # (orbm_project_points has no valid flag)
    want = {"mode0": pp | {R.ACCEPTED_WIDE}, "mode1": pp, "mode2": pp, "last": {R.INVALID, R.BEHIND, R.OUT_U, R.OUT_V, R.ACCEPTED},
            "kf": A - {R.BEHIND, R.VIEW_ANGLE}, "sim3": A, "pair": A - {R.VIEW_ANGLE}}
    for form, codes in want.items():
        assert SEEN.get(form, set()) == codes, (form, sorted(SEEN.get(form, set())))
    for form in ("mode0", "mode1", "mode2", "kf", "sim3", "pair"):
        assert SEEN[form + "_clamp"] == {R.LEVEL_IN, R.LEVEL_LOW, R.LEVEL_HIGH}, form
