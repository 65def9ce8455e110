"""The constructed selection cases of tests/selection_scenes.py against the C oracle's literal loops (no GPU): what every case
declares as its best / second candidate, and the acceptance rule restated in numpy float32, must be what
oracle.search_projection_seq, search_by_bow, search_for_initialization, search_window and search_fuse compute.  The GPU module
(tests/test_gpu_selection_edges.py) then holds the kernels against both.  The last test checks that the scenes reached every
branch the cases are about."""
import numpy as np
import pytest

import oracle
import selection_scenes as S

REACHED = set()


def _reach(kind, rule, sc, mq):
    """A case counts as reached under a rule; where a match was due the expectation holds one."""
    REACHED.update((kind, rule, t) for t in sc.tags())
    for i in range(sc.nq):
        if sc.q[i][1].want:
            assert mq[i] >= 0, sc.island_of[i].name


def same_ints(got, want, sc=None, what=""):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if not np.array_equal(g, w):
            bad = [int(i) for i in np.nonzero(g != w)[0][:5]] if g.shape == w.shape and g.ndim else []
            names = [sc.island_of[i].name for i in bad] if sc is not None and g.shape == (sc.nq,) else []
            raise AssertionError(f"{what}: differs at {bad} {names}: got {g[bad] if bad else g}, want {w[bad] if bad else w}")


def oracle_projection(sc, rule, th, ratio, takes):
    return oracle.search_projection_seq(sc.windows(), sc.qdesc, sc.qangle, sc.takes(takes), sc.kps, sc.desc, S.BOUNDS, None, None, th, ratio,
                                        rule == S.SAME_LEVEL, False)


def oracle_init(sc, ratio, check=False):
    k1, prev = sc.init_queries()
    return oracle.search_for_initialization(k1, sc.qdesc, sc.kps, sc.desc, prev, S.BOUNDS, sc.window, ratio, check)


def oracle_bow(sc, kf_kf, ratio):
    fv1, fv2 = sc.bow()
    return oracle.search_by_bow(fv1, np.ones(sc.nq, np.uint8), sc.qdesc, sc.qangle, fv2, np.ones(len(sc.kps), np.uint8), sc.desc,
                                sc.kps["angle"], kf_kf, ratio, False)


@pytest.mark.parametrize("takes", [1, 0])
@pytest.mark.parametrize("rule,th,ratio,kind", S.PROJECTION_SCENES)
def test_projection_family(rule, th, ratio, kind, takes):
    sc = S.scene(kind, rule, th, ratio) if kind == "core" else S.scene(kind)
    want = sc.expect_projection(rule, th, ratio, takes)
    same_ints(oracle_projection(sc, rule, th, ratio, takes), want, sc, "oracle vs expectation")
    if takes:
        _reach("projection", rule, sc, want[1])
    else:
        REACHED.add(("projection", rule, "takes0"))
        if kind == "core" and th <= S.TH_HIGH:      # (the claim cases: several queries accepted on one slot, match_kp holds the last)
            assert (np.bincount(want[1][want[1] >= 0]) > 1).any()


@pytest.mark.parametrize("offset", S.CLAIM_OFFSETS)
@pytest.mark.parametrize("rule,th,ratio", [(S.BEST, S.TH_HIGH, 0.6), (S.SAME_LEVEL, S.TH_HIGH, 0.6), (S.INIT, S.TH_LOW, 0.9)])
def test_claims_either_side_of_a_batch(rule, th, ratio, offset):
    sc = S.scene("claims", rule, th, ratio, offset)
    if rule == S.INIT:
        m12, nm, acc = sc.expect_init(ratio)
        got = oracle_init(sc, ratio)
        same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
        assert nm == 5
    else:
        for takes in (1, 0):
            want = sc.expect_projection(rule, th, ratio, takes)
            same_ints(oracle_projection(sc, rule, th, ratio, takes), want, sc, "oracle vs expectation")
            assert want[2] == 5 and (len(set(want[1][want[1] >= 0])) == (5 if takes else 2))
    REACHED.add(("claims", rule, offset))


@pytest.mark.parametrize("kind,arg", [("chain", 47), ("chain", 48), ("many", 2048), ("many", 2049)])
@pytest.mark.parametrize("rule,th,ratio", [(S.BEST, S.TH_HIGH, 0.6), (S.INIT, S.TH_LOW, 0.9)])
def test_fixed_point_limits(rule, th, ratio, kind, arg):
    sc = S.scene(kind, rule, th, ratio, arg)
    n = arg if kind == "chain" else 16
    if rule == S.INIT:
        m12, nm, _ = sc.expect_init(ratio)
        got = oracle_init(sc, ratio)
        same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
    else:
        want = sc.expect_projection(rule, th, ratio)
        same_ints(oracle_projection(sc, rule, th, ratio, 1), want, sc, "oracle vs expectation")
        m12, nm = want[1], want[2]
    assert nm == n and np.array_equal(m12[-n:], np.arange(n)) and (m12[:-n] == -1).all()
    REACHED.add(("limits", rule, kind, arg))


@pytest.mark.parametrize("kind,ratio", S.INIT_SCENES)
def test_search_for_initialization(kind, ratio):
    sc = S.scene(kind, S.INIT, S.TH_LOW, ratio)
    m12, nm, acc = sc.expect_init(ratio)
    got = oracle_init(sc, ratio)
    same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
    _reach("init", S.INIT, sc, acc)
    if kind == "core":
        assert (acc >= 0).sum() == nm + 1           # one steal in the scene: one acceptor more than matches


@pytest.mark.parametrize("arg", [1024, 1025])
def test_initialization_list_region(arg):
    sc = S.scene("init_lists", S.INIT, S.TH_LOW, 0.9, arg)
    m12, nm, acc = sc.expect_init(0.9)
    got = oracle_init(sc, 0.9)
    same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
    assert nm == 2
    REACHED.add(("init_lists", arg))


@pytest.mark.parametrize("k", [7, 8])
def test_initialization_acceptors_of_one_slot(k):
    sc = S.scene("init_acceptors", S.INIT, S.TH_LOW, 0.9, k)
    m12, nm, acc = sc.expect_init(0.9)
    got = oracle_init(sc, 0.9)
    same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
    assert nm == 1 and (acc >= 0).all() and m12[-1] == 0
    REACHED.add(("init_acceptors", k))


@pytest.mark.parametrize("tip", ["keep", "drop"])
def test_initialization_stolen_matches_count_in_the_histogram(tip):
    sc, m12, nm = S.rotation_scene(tip)
    got = oracle_init(sc, 0.9, True)
    same_ints((got[0], got[2]), (m12, nm), sc, "oracle vs expectation")
    plain = oracle_init(sc, 0.9, False)
    assert plain[2] == (nm if tip == "keep" else nm + 1)
    REACHED.add(("rotation", tip))


@pytest.mark.parametrize("kf_kf", [False, True])
@pytest.mark.parametrize("ratio", S.RATIOS)
def test_search_by_bow(ratio, kf_kf):
    th = S.TH_LOW - 1 if kf_kf else S.TH_LOW
    sc = S.scene("bow", S.RATIO, th, ratio)
    want = sc.expect_bow(kf_kf, ratio)
    same_ints(oracle_bow(sc, kf_kf, ratio), want, sc, "oracle vs expectation")
    _reach("bow", S.RATIO, sc, want[0])
    REACHED.add(("bow", "kf_kf", kf_kf))


@pytest.mark.parametrize("kf_kf", [False, True])
def test_search_by_bow_nodes(kf_kf):
    a, want = S.bow_special(kf_kf)
    z1, z2 = np.zeros(len(a["desc1"]), np.float32), np.zeros(len(a["desc2"]), np.float32)
    got = oracle.search_by_bow(a["fv1"], a["valid1"], a["desc1"], z1, a["fv2"], a["valid2"], a["desc2"], z2, kf_kf, 0.6, False)
    same_ints(got, want, None, "oracle vs expectation")
    REACHED.add(("bow_nodes", kf_kf))


@pytest.mark.parametrize("init_dist", [256, S.INT_MAX])
@pytest.mark.parametrize("kind", ["window", "lengths", "long_plain"])
def test_uncoupled_window_and_fuse(kind, init_dist):
    sc = S.scene(kind)
    want = sc.expect_window(init_dist)
    got = oracle.search_window(sc.windows(), sc.qdesc, sc.kps, sc.desc, S.BOUNDS, None, None, init_dist)
    same_ints(got, want, sc, "search_window: oracle vs expectation")
    if init_dist == 256:
        same_ints(oracle.search_fuse(sc.windows(), sc.qdesc, sc.kps, sc.desc, S.BOUNDS), (want[0], want[4]), sc, "search_fuse: oracle vs expectation")
    REACHED.update(("window", init_dist, t) for t in sc.tags())
    assert (want[4] >= 0).sum() >= sc.nq - 3


def test_every_case_was_reached():
    """Across this module (its tests run in file order) every branch the issue lists was set up under every rule that has it."""
    for rule in (S.BEST, S.SAME_LEVEL):
        missing = {t for t in S.REQUIRED if ("projection", rule, t) not in REACHED} - ({t for t in S.REQUIRED if t.startswith("ratio_")} if rule == S.BEST else set())
        assert not missing, (rule, missing)
        assert ("projection", rule, "takes0") in REACHED
    for kind, rule in (("init", S.INIT), ("bow", S.RATIO)):
        missing = {t for t in S.REQUIRED if (kind, rule, t) not in REACHED}
        assert not missing, (kind, missing)
    for t in ("init_steal", "init_equal", "init_left_out_of_second", "init_level0_only"):
        assert ("init", S.INIT, t) in REACHED, t
    for L in S.SHORT_LENGTHS + S.LONG_LENGTHS:
        for kind, rule in (("projection", S.BEST), ("projection", S.SAME_LEVEL), ("init", S.INIT), ("bow", S.RATIO)):
            assert (kind, rule, f"len_{L}") in REACHED, (kind, L)
        assert ("window", 256, f"len_{L}") in REACHED and ("window", S.INT_MAX, f"len_{L}") in REACHED
    for w in ("winner_first", "winner_8", "winner_9", "winner_last", "steps4", "steps5"):
        assert ("projection", S.BEST, w) in REACHED and ("init", S.INIT, w) in REACHED and ("window", 256, w) in REACHED, w
    for lv in ("levels_0_0", "levels_3_4", "levels_15_15", "levels_15_14"):
        assert ("projection", S.SAME_LEVEL, lv) in REACHED and ("window", 256, lv) in REACHED, lv
    for rule in (S.BEST, S.SAME_LEVEL, S.INIT):
        assert all(("claims", rule, o) in REACHED for o in S.CLAIM_OFFSETS)
        if rule != S.SAME_LEVEL:
            assert all(("limits", rule, k, a) in REACHED for k, a in (("chain", 47), ("chain", 48), ("many", 2048), ("many", 2049)))
    assert all(t in REACHED for t in (("init_lists", 1024), ("init_lists", 1025), ("init_acceptors", 7), ("init_acceptors", 8),
                                      ("rotation", "keep"), ("rotation", "drop"), ("bow", "kf_kf", False), ("bow", "kf_kf", True),
                                      ("bow_nodes", False), ("bow_nodes", True)))
    # each ratio rule met a pair that a double product decides the other way
    assert ("projection", S.SAME_LEVEL, "ratio_f32_vs_double") in REACHED and ("bow", S.RATIO, "ratio_f32_vs_double") in REACHED
    assert ("init", S.INIT, "ratio_f32_vs_double") in REACHED
