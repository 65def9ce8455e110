"""GPU: the selection core of orbm_search.hip at its decision edges -- wave_topk / wave_topk_regs, select_two's three routes,
accepts_projection / accepts_initialization, the claim table of k_resolve<0|1>, the fixed points k_resolve_par /
k_resolve_init_par and k_win_best's best / second -- on the constructed cases of tests/selection_scenes.py.  Every entry that
runs the core is held, as integers, against BOTH the C oracle's literal loop and the case's own declared expectation (which
tests/test_cpu_selection.py holds against the oracle on the CPU), as host arrays and on a resident frame, under both resolvers.

Where the route matters the test asks orbm_debug_last_resolver_iterations which one ran.  From k_resolve_par's loop: query i of
a dependency chain settles in iteration i, the first iteration without a change is number c for a chain of c queries, and the
kernel reports that number + 1; RES_MAXIT = 48 iterations run at most.  So a chain of 47 reports 48 and a chain of 48 does
not converge: -1, and the call repeats on k_resolve.  The same holds for k_resolve_init_par, which also gives up (-1) when a
keypoint has more than init_c = 7 acceptors in one iteration.

Octaves: a candidate entry holds its keypoint's octave in four bits, so the entries refuse a frame with an octave outside
0..15 (ORBX_ERR_ARG, "octave out of range"); octave 15 is searched like any other (the levels_15_* cases).

Mutations of orbm_search.hip tried on a scratch copy; each fails the tests named (and passes the rest of the module):
  best <= th -> < in accepts_projection           th_eq and its kin: test_projection_family[*-core-*] (all 11 rules), test_search_by_bow
  best <= th -> < in accepts_initialization       test_search_for_initialization[core-*]
  the three ratio products in double              test_projection_family[same_level-*-0.7 / 0.9-core], test_search_by_bow[0.6 / 0.8],
                                                  test_search_for_initialization[core-0.6 / 0.8] (the ratio_f32_vs_double pairs)
  found == 0: scan = d7 <= th -> <                found0_scan_d7_eq_th: test_projection_family[*-core-1], test_search_by_bow,
                                                  test_search_for_initialization[core-*]
  the d7 shortcut taken without `accepts`         found1_scan_all_blocked / _second_passes: test_projection_family[same_level-*-core-1],
                                                  test_search_by_bow, test_search_for_initialization[core-*] (ACCEPT_BEST never takes
                                                  the shortcut: it wants one candidate)
  key > prev -> >= in wave_topk                   lists beyond 256: test_projection_family[same_level-95-0.6-long-*], test_search_by_bow,
                                                  test_search_for_initialization[long], test_initialization_list_region
  st > dist -> >= in the initialization rule      test_search_for_initialization[core-*], test_claims_either_side_of_a_batch[init-*],
                                                  test_fixed_point_limits[init-*]
  k < C -> <= in claim                            test_initialization_acceptors_of_one_slot[8]: same matches, but the fixed point
                                                  reports 2 iterations where it has to give up (-1); only the iteration count shows it
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import selection_scenes as S
from orb_slam2_e_amd import Frame, ORBmatcher, Points, View
from orb_slam2_e_amd._lib import OrbxError, lib
from test_cpu_selection import oracle_bow, oracle_init, oracle_projection, same_ints

ERR_ARG = -1


def iterations(resolver):
    """What the last call's fixed point reported (None under the forced sequential resolver, which does not report)."""
    return lib().orbm_debug_last_resolver_iterations() if resolver == "parallel fixed point" else None


def device_projection(sc, rule, th, ratio, takes, resolver=None):
    """search_projection on host arrays and on a resident frame -> the two results (and the host call's iteration count)."""
    m = ORBmatcher(ratio, False)
    a = (sc.windows(), sc.qdesc, sc.qangle, sc.takes(takes))
    host = m.search_projection(*a, sc.kps, sc.desc, S.BOUNDS, th_accept=th, ratio_same_level=rule == S.SAME_LEVEL)
    it = iterations(resolver)
    f = Frame(sc.kps, sc.desc, S.BOUNDS)
    res = m.frame_search_projection(f, *a, th_accept=th, ratio_same_level=rule == S.SAME_LEVEL)
    f.close()
    return host, res, it


def device_init(sc, ratio, check=False, resolver=None):
    m = ORBmatcher(ratio, check)
    k1, prev = sc.init_queries()
    host = m.SearchForInitialization(k1, sc.qdesc, sc.kps, sc.desc, prev, S.BOUNDS, sc.window)
    it = iterations(resolver)
    f = Frame(sc.kps, sc.desc, S.BOUNDS)
    res = m.frame_search_for_initialization(f, sc.kps, k1, sc.qdesc, prev, sc.window)
    f.close()
    return host, res, it


def check_projection(sc, rule, th, ratio, takes, resolver):
    want = sc.expect_projection(rule, th, ratio, takes)
    ref = oracle_projection(sc, rule, th, ratio, takes)
    host, res, it = device_projection(sc, rule, th, ratio, takes, resolver)
    for got, name in ((host, "host arrays"), (res, "resident frame")):
        same_ints(got, ref, sc, name + " vs oracle"); same_ints(got, want, sc, name + " vs expectation")
    return want, it


def check_init(sc, ratio, resolver, check=False, want=None):
    if want is None:
        want = sc.expect_init(ratio)[:2]
    ref = oracle_init(sc, ratio, check)
    host, res, it = device_init(sc, ratio, check, resolver)
    for got, name in ((host, "host arrays"), (res, "resident frame")):
        same_ints(got, ref, sc, name + " vs oracle"); same_ints((got[0], got[2]), want, sc, name + " vs expectation")
    return want, it


@pytest.mark.parametrize("takes", [1, 0])
@pytest.mark.parametrize("rule,th,ratio,kind", S.PROJECTION_SCENES)
def test_projection_family(rule, th, ratio, kind, takes, resolver):
    """Thresholds, ratio pairs, ties, list lengths, the three routes of select_two and claims under ACCEPT_BEST and
    ACCEPT_RATIO_SAME_LEVEL; takes = 0: nothing blocks.  `long`: lists beyond the 256-entry region (exact count / scan / fill)."""
    sc = S.scene(kind, rule, th, ratio) if kind == "core" else S.scene(kind)
    check_projection(sc, rule, th, ratio, takes, resolver)


@pytest.mark.parametrize("offset", S.CLAIM_OFFSETS)
@pytest.mark.parametrize("rule,th,ratio", [(S.BEST, S.TH_HIGH, 0.6), (S.SAME_LEVEL, S.TH_HIGH, 0.6), (S.INIT, S.TH_LOW, 0.9)])
def test_claims_either_side_of_a_batch(rule, th, ratio, offset, resolver):
    """Two and three queries want one slot, starting at query 62 .. 65 of the call: the lowest index keeps it, the others take their
    second choice; with takes = 0 all are accepted on it and match_kp holds the last."""
    sc = S.scene("claims", rule, th, ratio, offset)
    if rule == S.INIT:
        check_init(sc, ratio, resolver)
        return
    for takes in (1, 0):
        want, it = check_projection(sc, rule, th, ratio, takes, resolver)
        assert want[2] == 5
        if it is not None:
            assert it == (4 if takes else 2)         # a chain of three queries; nothing to settle when nothing blocks


@pytest.mark.parametrize("kind,arg,reports", [("chain", 47, 48), ("chain", 48, -1), ("many", 2048, 17), ("many", 2049, 17)])
@pytest.mark.parametrize("rule,th,ratio", [(S.BEST, S.TH_HIGH, 0.6), (S.INIT, S.TH_LOW, 0.9)])
def test_fixed_point_limits(rule, th, ratio, kind, arg, reports, resolver):
    """The longest dependency chain that still converges and one longer (the call then repeats on k_resolve); 2048 queries (the
    fixed point keeps RES_T * RES_QREG of them in registers) and 2049 (the last one, which is matched, lives in global memory)."""
    sc = S.scene(kind, rule, th, ratio, arg)
    _, it = check_init(sc, ratio, resolver) if rule == S.INIT else check_projection(sc, rule, th, ratio, 1, resolver)
    if it is not None:
        assert it == reports


@pytest.mark.parametrize("kind,ratio", S.INIT_SCENES)
def test_search_for_initialization(kind, ratio, resolver):
    sc = S.scene(kind, S.INIT, S.TH_LOW, ratio)
    check_init(sc, ratio, resolver)


@pytest.mark.parametrize("arg", [1024, 1025])
def test_initialization_list_region(arg, resolver):
    """Lists of 1024 entries fill SearchForInitialization's region; one more sends the call to the exact route."""
    check_init(S.scene("init_lists", S.INIT, S.TH_LOW, 0.9, arg), 0.9, resolver)


@pytest.mark.parametrize("k,reports", [(7, 2), (8, -1)])
def test_initialization_acceptors_of_one_slot(k, reports, resolver):
    """init_c = 7 acceptors of one keypoint fit the fixed point's per-slot list (their selections never change: 2 iterations);
    with 8 it gives up and the call repeats on k_resolve<1>."""
    _, it = check_init(S.scene("init_acceptors", S.INIT, S.TH_LOW, 0.9, k), 0.9, resolver)
    if it is not None:
        assert it == reports


@pytest.mark.parametrize("tip", ["keep", "drop"])
def test_initialization_stolen_matches_count_in_the_histogram(tip, resolver):
    sc, m12, nm = S.rotation_scene(tip)
    check_init(sc, 0.9, resolver, True, (m12, nm))


def _bow_frames(sc):
    k1, _ = sc.init_queries()
    return Frame(k1, sc.qdesc, S.BOUNDS), Frame(sc.kps, sc.desc, S.BOUNDS)


@pytest.mark.parametrize("kf_kf", [False, True])
@pytest.mark.parametrize("ratio", S.RATIOS)
def test_search_by_bow(ratio, kf_kf, resolver):
    """ACCEPT_RATIO at TH_LOW (Frame form) and below it (KeyFrame form); member lists of 1 .. 300 (wave_topk's two forms either
    side of 256); claims inside one node either side of a 64-query batch."""
    sc = S.scene("bow", S.RATIO, S.TH_LOW - 1 if kf_kf else S.TH_LOW, ratio)
    want, ref = sc.expect_bow(kf_kf, ratio), oracle_bow(sc, kf_kf, ratio)
    m = ORBmatcher(ratio, False)
    fv1, fv2 = sc.bow()
    v1, v2 = np.ones(sc.nq, np.uint8), np.ones(len(sc.kps), np.uint8)
    host = m.SearchByBoW(fv1, v1, sc.qdesc, sc.qangle, fv2, v2, sc.desc, sc.kps["angle"], kf_kf)
    f1, f2 = _bow_frames(sc)
    res = m.frame_search_by_bow(f1, fv1, v1, f2, fv2, v2, kf_kf)
    f1.close(); f2.close()
    for got, name in ((host, "host arrays"), (res, "resident frames")):
        same_ints(got, ref, None, name + " vs oracle"); same_ints(got, want, None, name + " vs expectation")


@pytest.mark.parametrize("kf_kf", [False, True])
def test_search_by_bow_nodes(kf_kf, resolver):
    """A node with one member on each side, nodes present on one side only, `valid` flags that empty a node on either side."""
    a, want = S.bow_special(kf_kf)
    z1, z2 = np.zeros(len(a["desc1"]), np.float32), np.zeros(len(a["desc2"]), np.float32)
    ref = oracle.search_by_bow(a["fv1"], a["valid1"], a["desc1"], z1, a["fv2"], a["valid2"], a["desc2"], z2, kf_kf, 0.6, False)
    m = ORBmatcher(0.6, False)
    host = m.SearchByBoW(a["fv1"], a["valid1"], a["desc1"], z1, a["fv2"], a["valid2"], a["desc2"], z2, kf_kf)
    kp = lambda n: np.zeros(n, oracle.KP_DTYPE)
    k1, k2 = kp(len(z1)), kp(len(z2))
    for k in (k1, k2):
        k["x"] = 100.0 + np.arange(len(k)); k["y"] = 100.0
    f1, f2 = Frame(k1, a["desc1"], S.BOUNDS), Frame(k2, a["desc2"], S.BOUNDS)
    res = m.frame_search_by_bow(f1, a["fv1"], a["valid1"], f2, a["fv2"], a["valid2"], kf_kf)
    f1.close(); f2.close()
    for got in (host, res):
        same_ints(got, ref, None, "vs oracle"); same_ints(got, want, None, "vs expectation")


@pytest.mark.parametrize("init_dist", [256, S.INT_MAX])
@pytest.mark.parametrize("kind", ["window", "lengths", "long_plain"])
def test_uncoupled_window_and_fuse(kind, init_dist):
    """k_win_best's own best / second rule: search_window from 256 and from INT_MAX (a candidate at 256 is then one like any other),
    search_fuse; host arrays and resident frame."""
    sc = S.scene(kind)
    want = sc.expect_window(init_dist)
    q = sc.windows()
    ref = oracle.search_window(q, sc.qdesc, sc.kps, sc.desc, S.BOUNDS, None, None, init_dist)
    m = ORBmatcher(0.6, False)
    f = Frame(sc.kps, sc.desc, S.BOUNDS)
    for got, name in ((m.search_window(q, sc.qdesc, sc.kps, sc.desc, S.BOUNDS, None, None, init_dist), "host arrays"),
                      (m.frame_search_window(f, q, sc.qdesc, None, init_dist), "resident frame")):
        same_ints(got, ref, sc, name + " vs oracle"); same_ints(got, want, sc, name + " vs expectation")
    if init_dist == 256:
        ref = oracle.search_fuse(q, sc.qdesc, sc.kps, sc.desc, S.BOUNDS)
        for got in (m.search_fuse(q, sc.qdesc, sc.kps, sc.desc, S.BOUNDS), m.frame_search_fuse(f, q, sc.qdesc)):
            same_ints(got, ref, sc, "fuse vs oracle"); same_ints(got, (want[0], want[4]), sc, "fuse vs expectation")
    f.close()


# ---------------------------------------------------------------------------------------------------- octaves
def _refused(call):
    with pytest.raises(OrbxError) as e:
        call()
    assert e.value.code == ERR_ARG and "octave out of range" in str(e.value)


@pytest.mark.parametrize("octave", [16, -1])
def test_entries_refuse_an_octave_outside_four_bits(octave):
    """Every entry whose candidate entries pack the octave: the host-array forms check the keypoints, the resident-frame forms
    and the whole-function forms the frame's octave range."""
    sc = S.scene("window")
    kps = sc.kps.copy()
    kps["octave"][len(kps) // 2] = octave
    q, n, nq = sc.windows(), len(kps), sc.nq
    k1, prev = sc.init_queries()
    m = ORBmatcher(0.6, False)
    _refused(lambda: m.search_projection(q, sc.qdesc, sc.qangle, sc.takes(), kps, sc.desc, S.BOUNDS))
    _refused(lambda: m.SearchForInitialization(k1, sc.qdesc, kps, sc.desc, prev, S.BOUNDS, 5))
    _refused(lambda: m.search_window(q, sc.qdesc, kps, sc.desc, S.BOUNDS))
    f = Frame(kps, sc.desc, S.BOUNDS)
    _refused(lambda: m.frame_search_projection(f, q, sc.qdesc, sc.qangle, sc.takes()))
    _refused(lambda: m.frame_search_for_initialization(f, kps, k1, sc.qdesc, prev, 5))
    _refused(lambda: m.frame_search_window(f, q, sc.qdesc))
    # the whole-function forms: one valid point in front of the camera is all they need to get as far as the check
    view = View(500.0, 500.0, 320.0, 240.0, 0.1, 40.0, float(np.log(np.float32(1.2))), np.float32(1.2) ** np.arange(8, dtype=np.float32))
    T = np.eye(4, dtype=np.float32)
    one = dict(valid=np.ones(1, np.uint8), pos=np.array([[0.0, 0.0, 2.0]], np.float32), desc=sc.qdesc[:1])
    rng = dict(min_distance=np.ones(1, np.float32), max_distance=np.full(1, 10.0, np.float32))
    nrm = dict(normal=np.array([[0.0, 0.0, -1.0]], np.float32))
    _refused(lambda: m.SearchByProjectionPoints(f, view, T, Points(**one, **rng, **nrm), None))
    _refused(lambda: m.SearchByProjectionLast(f, view, T, T, Points(**one, octave=np.zeros(1, np.int32), angle=np.zeros(1, np.float32)), None, 7.0, True))
    _refused(lambda: m.SearchByProjectionKeyFrame(f, view, T, Points(**one, **rng, angle=np.zeros(1, np.float32)), None, 7.0, 100))
    _refused(lambda: m.SearchByProjectionSim3(f, view, T, Points(**one, **rng, **nrm), None, 10))
    full = lambda fr: Points(np.ones(fr.n, np.uint8), np.tile(one["pos"], (fr.n, 1)), sc.desc[:fr.n], min_distance=np.ones(fr.n, np.float32),
                             max_distance=np.full(fr.n, 10.0, np.float32))
    g = Frame(sc.kps, sc.desc, S.BOUNDS)
    R, t = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    _refused(lambda: m.SearchBySim3Whole(f, g, view, T, T, 1.0, R, t, full(f), full(g), 7.5))
    _refused(lambda: m.SearchBySim3Whole(g, f, view, T, T, 1.0, R, t, full(g), full(f), 7.5))
    # the same calls on the frame as it was are accepted
    assert m.SearchByProjectionSim3(g, view, T, Points(**one, **rng, **nrm), None, 10)[2] >= 0
    assert m.SearchBySim3Whole(g, g, view, T, T, 1.0, R, t, full(g), full(g), 7.5)[1] >= 0
    f.close(); g.close()
