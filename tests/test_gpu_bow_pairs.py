"""orbm_frame_search_by_bow_pairs on the device: every pair's (match12, match21, nmatches) equals BOTH oracle.search_by_bow and the
single orbm_frame_search_by_bow call, integer for integer, under the `resolver` fixture's two settings.  The scenes are those of
tests/bow_pairs_scenes.py (checked on the oracle alone by tests/test_cpu_bow_pairs.py); a Side that stands in several pairs is ONE
resident frame.  Host waits: 0 when no pair has a query, 1 on the common path, one more per pair the fixed point gives up on;
under the forced sequential resolver every pair with a query takes the single-pair path, one wait each."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bow_pairs_scenes as B
from orb_slam2_e_amd import ORBmatcher
from orb_slam2_e_amd._lib import OrbxError, lib
from orb_slam2_e_amd.matcher import _CBowPair
from test_cpu_selection import same_ints

ERR_ARG, ERR_UNSUPPORTED = -1, -5
PARALLEL = "parallel fixed point"


@pytest.fixture(scope="module", autouse=True)
def frames():
    yield
    B.close_frames()


@pytest.fixture(scope="module")
def scenes():
    """every scene built once for the module (its oracle rows are cached in the Pair)"""
    cache = {}

    def get(name, make):
        if name not in cache:
            cache[name] = make()
        return cache[name]
    return get


_SINGLE = {}
LAST = {}


def single(p, kf_kf, ratio, ori, resolver):
    """the single call's rows for the pair, once per setting"""
    key = (id(p), kf_kf, ratio, ori, resolver)
    if key not in _SINGLE:
        _SINGLE[key] = (p, ORBmatcher(ratio, ori).frame_search_by_bow(*p.args(), kf_kf))
    return _SINGLE[key][1]


def run(pairs, kf_kf, ratio, ori, resolver):
    """the batch call; checks every pair against the oracle and the single call.  Returns (rows, host waits of the batch call)."""
    got = ORBmatcher(ratio, ori).frame_search_by_bow_pairs([p.args() for p in pairs], kf_kf)
    waits = ORBmatcher.last_bow_pairs_waits()
    LAST["iterations"] = lib().orbm_debug_last_resolver_iterations()      # (read before the single calls below overwrite it)
    assert len(got) == len(pairs)
    for k, (p, g) in enumerate(zip(pairs, got)):
        same_ints(g, p.oracle(kf_kf, ratio, ori), None, f"pair {k} ({p.name}) vs oracle")
        same_ints(g, single(p, kf_kf, ratio, ori, resolver), None, f"pair {k} ({p.name}) vs the single call")
    return got, waits


def expected_waits(pairs, resolver, unsettled=0):
    active = sum(1 for p in pairs if p.nqueries() and p.s2.n)
    if resolver == PARALLEL:
        return (1 + unsettled) if active else 0
    return active


@pytest.mark.parametrize("kf_kf", [False, True])
def test_decision_edges_in_one_batch(kf_kf, resolver, scenes):
    """selection_scenes' BoW scene (list lengths 1 .. 300 either side of wave_topk's 256, claims at queries 62 - 65 of a node) and
    bow_special in the same batch, with their hand-made expectations."""
    sel, want_sel = scenes(("selection", kf_kf), lambda: B.selection_pair(kf_kf))
    spec, want = scenes(("special", kf_kf), lambda: B.special_pair(kf_kf))
    pairs = [sel, spec, scenes("case0", lambda: B.case_pair(0))]
    got, waits = run(pairs, kf_kf, 0.6, False, resolver)
    same_ints(got[0], want_sel, None, "selection scene vs expectation")
    same_ints(got[1], want, None, "special scene vs expectation")
    assert waits == expected_waits(pairs, resolver)


def test_placement_does_not_matter(resolver, scenes):
    """the same pair alone, first / middle / last of three, and in a batch listed in reverse: the same bytes"""
    a, b, c = (scenes(f"case{s}", lambda s=s: B.case_pair(s)) for s in (0, 1, 2))
    alone, waits = run([a], False, 0.75, True, resolver)
    assert waits == 1
    for order in ([a, b, c], [b, a, c], [b, c, a], [c, b, a]):
        got, waits = run(order, False, 0.75, True, resolver)
        same_ints(got[order.index(a)], alone[0], None, "placement")
        assert waits == expected_waits(order, resolver)


def test_sixty_four_pairs_and_one_more(resolver, scenes):
    small = [scenes(("small", s), lambda s=s: B.case_pair(20 + s, 60, 70, 4)) for s in range(8)]
    got, waits = run([small[k % 8] for k in range(64)], True, 0.75, True, resolver)
    assert waits == (1 if resolver == PARALLEL else 64)
    assert all(g[2] > 5 for g in got)
    with pytest.raises(OrbxError) as e:
        ORBmatcher(0.75, True).frame_search_by_bow_pairs([small[0].args()] * 65, True)
    assert e.value.code == ERR_UNSUPPORTED


def test_pairs_without_a_query_between_ordinary_pairs(resolver, scenes):
    """no common node / an empty frame: rows all -1, count 0, no part in the launch; the neighbours are untouched"""
    a, b = scenes("case0", lambda: B.case_pair(0)), scenes("case1", lambda: B.case_pair(1))
    none, empty = scenes("disjoint", B.disjoint_pair), scenes("empty", B.empty_pair)
    pairs = [a, none, empty, b]
    got, waits = run(pairs, False, 0.75, True, resolver)
    for g in got[1:3]:
        assert g[2] == 0 and (g[0] == -1).all() and (g[1] == -1).all()
    assert len(got[2][0]) == 0 and len(got[1][0]) == none.s1.n
    assert waits == expected_waits(pairs, resolver) == (1 if resolver == PARALLEL else 2)


@pytest.mark.parametrize("kf_kf", [False, True])
def test_counters_of_batches_that_launch_nothing(kf_kf, resolver, scenes):
    none, empty = scenes("disjoint", B.disjoint_pair), scenes("empty", B.empty_pair)
    run([scenes("case0", lambda: B.case_pair(0))], kf_kf, 0.75, True, resolver)       # leaves a count behind
    got, waits = run([none, empty, none], kf_kf, 0.75, True, resolver)
    assert waits == 0 and all(g[2] == 0 for g in got)
    assert ORBmatcher(0.75, True).frame_search_by_bow_pairs([], kf_kf) == [] and ORBmatcher.last_bow_pairs_waits() == 0


def test_ten_ordinary_pairs_wait_once(resolver, scenes):
    pairs = [scenes(f"case{s}", lambda s=s: B.case_pair(s)) for s in range(10)]
    _, waits = run(pairs, False, 0.75, True, resolver)
    assert waits == (1 if resolver == PARALLEL else 10)


def test_a_query_beyond_the_registers_beside_a_small_pair(resolver, scenes):
    """2,049 valid queries (RES_T * RES_QREG + 1: the last one lives in global memory) beside a pair of 5, in both orders: the
    grid of the list kernel and the LDS of the resolver are sized for the larger pair wherever it stands."""
    many = scenes("many", B.many_pair)
    tiny = scenes("tiny", lambda: B.case_pair(59, 7, 9, 1))
    assert tiny.nqueries() == 5
    for order in ([many, tiny], [tiny, many]):
        got, waits = run(order, False, 0.75, True, resolver)
        assert waits == expected_waits(order, resolver)
    assert got[1][2] > 300


def test_largest_second_frame_is_not_the_first_pair_s(resolver, scenes):
    """the launch's dynamic LDS comes from the batch's largest ns, each workgroup lays out its own"""
    small = scenes("case0", lambda: B.case_pair(0))
    big = scenes("big", lambda: B.case_pair(3, 500, 700, 12))
    sel = scenes(("selection", False), B.selection_pair)[0]         # 4,324 keypoints in the second frame
    run([small, big, sel, small], False, 0.6, False, resolver)


def test_shared_frames(resolver, scenes):
    """one frame2 in all of 4 pairs (relocalisation), one frame1 in all of 4 pairs (loop closing): frames are only read"""
    reloc = scenes("shared_second", lambda: B.shared_second([0, 1, 2, 3]))
    loop = scenes("shared_first", lambda: B.shared_first([0, 1, 2, 3]))
    assert len({id(p.s2.frame()) for p in reloc}) == 1 and len({id(p.s1.frame()) for p in loop}) == 1
    run(reloc, False, 0.75, True, resolver)
    run(loop, True, 0.75, True, resolver)
    run(reloc + loop, True, 0.75, True, resolver)


def test_rotation_check_is_per_pair(resolver, scenes):
    """pairs whose dominant angle offsets differ (one second frame turned by 100 degrees), with the check on: a histogram or a
    three-maxima result shared between workgroups would reject the wrong matches"""
    p = scenes("case0", lambda: B.case_pair(0))
    t = scenes("turned", lambda: B.turned(p, 100))
    q = scenes("case1", lambda: B.case_pair(1))
    got, _ = run([p, t, q, t, p], False, 0.75, True, resolver)
    assert not np.array_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("nchain,reports", [(B.RES_MAXIT - 1, B.RES_MAXIT), (B.RES_MAXIT + 1, -1)])
def test_a_pair_that_does_not_settle(nchain, reports, resolver, scenes):
    """A chain of 49 queries under the ratio rule outlasts RES_MAXIT = 48 iterations, one of 47 settles in 48.  Alone, the single
    call says which; between two ordinary pairs all three results are right, and the unsettled pair costs one more wait."""
    chain = scenes(("chain", nchain), lambda: B.chain_pair(nchain))
    a, b = scenes("case0", lambda: B.case_pair(0)), scenes("case1", lambda: B.case_pair(1))
    m = ORBmatcher(0.75, False)
    res = m.frame_search_by_bow(*chain.args(), False)
    if resolver == PARALLEL:
        assert lib().orbm_debug_last_resolver_iterations() == reports
    same_ints(res, chain.oracle(False, 0.75, False), None, "the chain alone")
    pairs = [a, chain, b]
    got, waits = run(pairs, False, 0.75, False, resolver)
    assert np.array_equal(got[1][0], np.arange(nchain)) and got[1][2] == nchain
    if resolver == PARALLEL:
        assert waits == (2 if reports < 0 else 1)
        assert LAST["iterations"] == reports          # the batch reports its slowest pair, or -1 if one gave up
        _, waits = run([chain], False, 0.75, False, resolver)           # a batch of one: the single call's waits
        assert waits == (2 if reports < 0 else 1)
    else:
        assert waits == 3


def test_refusals_with_frames(scenes):
    """a feature index out of range in ANY pair fails the whole call before anything is written"""
    a, b = scenes("case0", lambda: B.case_pair(0)), scenes("case1", lambda: B.case_pair(1))
    bad_items = b.s1.fv[2].copy(); bad_items[-1] = b.s1.n
    bad = (b.s1.frame(), (b.s1.fv[0], b.s1.fv[1], bad_items), b.s1.valid, b.s2.frame(), b.s2.fv, b.s2.valid)
    m = ORBmatcher(0.75, True)
    m.frame_search_by_bow_pairs([a.args()], False)
    assert ORBmatcher.last_bow_pairs_waits() >= 1
    with pytest.raises(OrbxError) as e:
        m.frame_search_by_bow_pairs([a.args(), bad], False)
    assert e.value.code == ERR_ARG and b"out of range" in lib().orbx_last_error()
    # ... and through the C ABI: the first pair's rows keep their sentinel
    arr = (_CBowPair * 2)()
    keep = []
    rows = [np.full(a.s1.n, -7, np.int32), np.full(b.s1.n, -7, np.int32)]
    for c, (f1, fv1, v1, f2, fv2, v2), row in zip(arr, (a.args(), bad), rows):
        keep.append([np.ascontiguousarray(x, np.int32) for x in fv1 + fv2] + [v1])
        n1, o1, i1, n2, o2, i2, v = keep[-1]
        c.frame1, c.nodes1, c.off1, c.items1, c.nn1, c.valid1 = f1._h.value, n1.ctypes.data, o1.ctypes.data, i1.ctypes.data, len(n1), v.ctypes.data
        c.frame2, c.nodes2, c.off2, c.items2, c.nn2, c.valid2 = f2._h.value, n2.ctypes.data, o2.ctypes.data, i2.ctypes.data, len(n2), None
        c.match12, c.match21 = row.ctypes.data, None
    nm = np.full(2, -7, np.int32)
    assert lib().orbm_frame_search_by_bow_pairs(arr, 2, 45, 0, 0.75, 1, nm.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert (nm == -7).all() and all((r == -7).all() for r in rows)
