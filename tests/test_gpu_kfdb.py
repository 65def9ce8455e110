"""The keyframe database on the device (orbm_kfdb_*, orbm_kfdb.hip) against tests/kfdb_reference.py: counts and first-word indices
with ==, scores with == on their raw bits.  Shapes are small and sit where the kernel can go wrong: K = 0, 1, 63, 64, 65, 130
keyframes (a wave, a workgroup of four waves, several workgroups; the grid's STRIDE -- a wave that goes on to a second slot -- starts
above 8,192 slots and has tests of its own at the end: a grid capped to one and three workgroups, and 8,300 slots), rows and queries of 0, 1, 63, 64, 65, 300 and 255, 256, 257 words
over a vocabulary of 1,000 (the 64-lane chunks of a row and the four chunks a wave takes at a time, the powers of two of the query's
binary search), words 0 and nwords - 1, dead slots in the middle and at the end.  A row and a query of 8,192 words cannot have strictly ascending ids below 1,000, so those two use a database
of their own over 20,000 words; so does the growth test, whose long rows fill the first pool in nine adds."""
import ctypes as C

import numpy as np
import pytest

import kfdb_reference as R
import kfdb_scenes as S
from orb_slam2_e_amd import KeyFrameDatabase
from orb_slam2_e_amd._lib import lib

pytestmark = pytest.mark.gpu

NWORDS = 1000
LENGTHS = (0, 1, 63, 64, 65, 300, 255, 256, 257)
ERR_ARG = -1


class Pair:
    """the device database and the restatement, fed the same operations"""
    def __init__(self, nwords=NWORDS):
        self.dev, self.ref = KeyFrameDatabase(nwords), R.ReferenceDatabase(nwords)

    def add(self, bow):
        s = self.dev.add(bow)
        assert s == self.ref.add(bow)
        return s

    def erase(self, slot):
        self.dev.erase(slot); self.ref.erase(slot)

    def clear(self):
        self.dev.clear(); self.ref.clear()

    def check_query(self, bow, what=""):
        """orbm_kfdb_query against the restatement; the wait counter says whether anything was launched"""
        common, first, score = self.dev.query(bow)
        live = self.dev.size()[0]
        assert self.dev.last_waits() == (1 if live and len(bow) else 0), what
        wc, wf, ws = self.ref.shared(bow)
        assert np.array_equal(common, wc), f"{what}: common {common} != {wc}"
        assert np.array_equal(first, wf), f"{what}: first"
        assert S.same_bits(score, ws), f"{what}: score bits differ at {np.nonzero(score.view(np.uint32) != ws.view(np.uint32))[0]}"
        return common, first, score


def edge_words(rng, n, nwords):
    """n distinct words; from 2 on, words 0 and nwords - 1 are among them"""
    if n < 2:
        return rng.choice(nwords, n, replace=False)
    return np.concatenate([[0, nwords - 1], 1 + rng.choice(nwords - 2, n - 2, replace=False)])


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 130])
def test_query_over_wave_workgroup_and_grid_boundaries(K):
    rng = np.random.default_rng(100 + K)
    p = Pair()
    for k in range(K):
        n = LENGTHS[(k + K) % len(LENGTHS)]
        p.add(S.bow_of(rng, edge_words(rng, n, NWORDS) if k % 3 == 0 else rng.choice(NWORDS, n, replace=False)))
    queries = [S.bow_of(rng, edge_words(rng, n, NWORDS)) for n in LENGTHS]
    for q in queries:
        p.check_query(q, f"K {K}, nq {len(q)}")
    if K >= 3:                                       # dead slots in the middle and at the end
        for s in sorted({K // 2, K // 2 + 1, K - 1}):
            p.erase(s)
        for q in queries:
            common, _, score = p.check_query(q, f"K {K} with dead slots, nq {len(q)}")
            assert common[K - 1] == -1 and common[K // 2] == -1 and score[K - 1] == 0 and not np.signbit(score[K - 1])
        assert p.dev.size() == (K - len({K // 2, K // 2 + 1, K - 1}), K)
    if K:                                            # every slot erased: nothing is launched, every row reads dead
        for s in range(K):
            if p.ref.kfs[s].alive:
                p.erase(s)
        common, first, score = p.check_query(queries[-1], "all erased")
        assert p.dev.last_waits() == 0 and (common == -1).all() and (first == -1).all() and not np.signbit(score).any()
    else:
        common, _, _ = p.check_query(queries[-1], "empty database")
        assert len(common) == 0 and p.dev.last_waits() == 0


def test_special_rows():
    rng = np.random.default_rng(7)
    p = Pair()
    qw = np.sort(edge_words(rng, 130, NWORDS))
    q = S.bow_of(rng, qw)
    others = np.setdiff1d(np.arange(NWORDS), qw)
    equal = p.add(dict(q))
    disjoint = p.add(S.bow_of(rng, rng.choice(others, 100, replace=False)))
    only_first = p.add(S.bow_of(rng, np.concatenate([[0], rng.choice(others[others > 0], 70, replace=False)])))           # the row's first word = the query's first
    only_last = p.add(S.bow_of(rng, np.concatenate([rng.choice(others, 70, replace=False), [NWORDS - 1]])))               # the row's last = the query's last
    mid = int(qw[64])
    lo_others = others[others < mid]
    row_last = p.add(S.bow_of(rng, np.concatenate([lo_others[:64], [mid]])))                                             # shares its 65th (last) word only
    empty = p.add({})
    common, first, score = p.check_query(q, "special rows")
    assert common[equal] == 130 and first[equal] == 0 and abs(float(score[equal]) - 1.0) < 1e-6
    for s in (disjoint, empty):
        assert common[s] == 0 and first[s] == -1 and score[s] == 0 and np.signbit(score[s])                              # -0.0f
    assert (common[only_first], first[only_first]) == (1, 0) and (common[only_last], first[only_last]) == (1, 129)
    assert (common[row_last], first[row_last]) == (1, 64) and score[row_last] > 0


def test_row_and_query_of_8192_words():
    rng = np.random.default_rng(8)
    p = Pair(20000)
    long_row = S.bow_of(rng, edge_words(rng, 8192, 20000))
    p.add(long_row)
    p.add(S.bow_of(rng, rng.choice(20000, 300, replace=False)))
    p.add(dict(long_row))
    assert len(long_row) == 8192
    common, _, score = p.check_query(long_row, "query of 8,192 = row of 8,192")
    assert common[0] == 8192 and common[2] == 8192 and abs(float(score[0]) - 1.0) < 1e-6
    p.check_query(S.bow_of(rng, edge_words(rng, 8192, 20000)), "another query of 8,192")
    p.check_query(S.bow_of(rng, rng.choice(20000, 65, replace=False)), "a short query against the long rows")


def test_clear_restarts_slots_and_growth_keeps_the_resident_rows():
    rng = np.random.default_rng(9)
    p = Pair(20000)
    for _ in range(5):
        p.add(S.bow_of(rng, rng.choice(20000, 200, replace=False)))
    p.erase(1)
    p.clear()
    assert p.dev.size() == (0, 0)
    q = S.bow_of(rng, edge_words(rng, 3000, 20000))
    assert len(p.check_query(q, "after clear")[0]) == 0 and p.dev.last_waits() == 0
    early = [S.bow_of(rng, np.concatenate([rng.choice(sorted(q), 150, replace=False), rng.choice(20000, 150)])) for _ in range(3)]
    assert [p.add(b) for b in early] == [0, 1, 2]                     # slots restart at 0
    before = p.check_query(q, "early rows")
    assert (before[0][:3] > 100).all()
    start = p.dev.reallocations()
    while p.dev.reallocations() < start + 2:                          # rows of 8,192 words: the pools double every few adds
        p.add(S.bow_of(rng, edge_words(rng, 8192, 20000)))
        assert p.dev.size()[1] < 64
    for _ in range(1100):                                             # and the slot table (1,024 slots at first), with empty rows
        p.dev.add({}); p.ref.add({})
    assert p.dev.reallocations() >= start + 3
    after = p.check_query(q, "after growth")
    assert np.array_equal(after[0][:3], before[0]) and np.array_equal(after[1][:3], before[1]) and S.same_bits(after[2][:3], before[2])


def test_score_list_and_refusals_that_need_a_resident_row():
    rng = np.random.default_rng(10)
    p = Pair()
    for k in range(70):
        p.add(S.bow_of(rng, rng.choice(NWORDS, LENGTHS[k % len(LENGTHS)], replace=False)))
    q = S.bow_of(rng, edge_words(rng, 300, NWORDS))
    _, _, column = p.check_query(q)
    slots = [69, 0, 5, 5, 64, 63, 5, 0] + list(range(70))             # repeats, and more than a workgroup's four
    got = p.dev.score(q, slots)
    assert p.dev.last_waits() == 1
    assert S.same_bits(got, column[slots]) and S.same_bits(got, p.ref.score(q, slots))
    assert len(p.dev.score(q, [])) == 0 and p.dev.last_waits() == 0  # n = 0: nothing launched
    empty_q = p.dev.score({}, [3, 4])
    assert p.dev.last_waits() == 0 and (empty_q == 0).all() and np.signbit(empty_q).all()
    L, h = lib(), p.dev._h
    p.erase(5)
    assert L.orbm_kfdb_erase(h, 5) == ERR_ARG and b"erased already" in L.orbx_last_error()           # a second erase
    assert L.orbm_kfdb_erase(h, 70) == ERR_ARG and L.orbm_kfdb_erase(h, -1) == ERR_ARG
    words, values = np.array(sorted(q), np.int32), np.array([q[w] for w in sorted(q)], np.float64)
    out = np.full(3, -7, np.float32)
    for bad in ([0, 5, 1], [0, 70, 1], [-1, 0, 1]):                                                   # dead, out of range
        lst = np.array(bad, np.int32)
        assert L.orbm_kfdb_score(h, words.ctypes.data, values.ctypes.data, len(words), lst.ctypes.data, 3, out.ctypes.data) == ERR_ARG
    assert (out == -7).all()
    assert p.dev.size() == (69, 70)
    p.check_query(q, "after the refusals")


def test_python_class_end_to_end_against_the_restatement():
    """about 100 keyframes, 10 queries (loop and relocalisation forms alternating, an id of 0 and repeated ids among them), erases in
    between, a random covisibility graph: candidates and all six persistent fields after every query"""
    ops = S.sequence(seed=21, nkf=100, nqueries=10, nplaces=5, words=120)
    dev, ref = KeyFrameDatabase(NWORDS), R.ReferenceDatabase(NWORDS)
    graph = {}
    best = lambda s: graph.get(s, [])
    nq = ncand = 0
    for op in ops:
        if op[0] == "add":
            s = dev.add(op[1])
            assert s == ref.add(op[1])
            graph[s] = op[2]
        elif op[0] == "erase":
            dev.erase(op[1]); ref.erase(op[1])
        else:
            if op[0] == "loop":
                got = dev.detect_loop_candidates(op[1], op[2], op[3], op[4], best)
                want = ref.detect_loop_candidates(op[1], op[2], op[3], op[4], best)
            else:
                got = dev.detect_relocalization_candidates(op[1], op[2], best)
                want = ref.detect_relocalization_candidates(op[1], op[2], best)
            assert dev.last_waits() == 1
            assert got == want, f"query {nq} ({op[0]}, id {op[2]})"
            for name, g, w in zip(dev.fields.NAMES, dev.fields.arrays(), ref.fields()):
                assert (S.same_bits(g, w) if g.dtype == np.float32 else np.array_equal(g, w)), f"query {nq}: {name}"
            nq += 1; ncand += len(got)
    assert nq == 10 and ncand > 0 and dev.size()[1] >= 100
    live = [k.slot for k in ref.kfs if k.alive][:20]
    assert S.same_bits(dev.score(ops[-1][1], live), ref.score(ops[-1][1], live))          # DetectLoop's minScore list


# ------------------------------------------------------------------------------------------------ the grid's stride
def _strided_database(rng):
    p = Pair()
    for k in range(130):
        p.add(S.bow_of(rng, rng.choice(NWORDS, LENGTHS[k % len(LENGTHS)], replace=False)))
    for s in (3, 4, 64, 65, 66, 129):                # dead rows that a wave meets on its first, a later and its last trip
        p.erase(s)
    return p


@pytest.mark.parametrize("blocks", [1, 3])
def test_waves_stride_over_slots_when_the_grid_is_capped(blocks):
    """With at most `blocks` workgroups (orbm_debug_kfdb_max_blocks) the 130 slots take 33 / 11 trips of the per-wave loop: a wave
    goes on to the next slot's row, dead rows among them, and the last trip is partly past the end.  Query and score list."""
    rng = np.random.default_rng(40 + blocks)
    p = _strided_database(rng)
    queries = [S.bow_of(rng, edge_words(rng, n, NWORDS)) for n in (1, 65, 300)]
    plain = [p.check_query(q, "default grid") for q in queries]
    live = [k.slot for k in p.ref.kfs if k.alive]
    slots = live[::-1] + live[:7] + [live[5]] * 3
    L = lib()
    prev = L.orbm_debug_kfdb_max_blocks(blocks)
    try:
        assert prev == 0 and L.orbm_debug_kfdb_max_blocks(blocks) == blocks
        for q, want in zip(queries, plain):
            got = p.check_query(q, f"{blocks} workgroups")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and S.same_bits(got[2], want[2])
            listed = p.dev.score(q, slots)
            assert p.dev.last_waits() == 1 and S.same_bits(listed, want[2][slots]) and S.same_bits(listed, p.ref.score(q, slots))
    finally:
        L.orbm_debug_kfdb_max_blocks(0)
    assert L.orbm_debug_kfdb_max_blocks(0) == 0


def test_default_grid_strides_beyond_8192_slots():
    """8,300 slots against the default grid of 2,048 workgroups x 4 waves: waves 0 .. 107 take a second slot.  Most rows are empty or
    one word (adds are cheap); real rows and dead slots sit on both sides of slot 8,192, so a wrong stride shows as a wrong row."""
    rng = np.random.default_rng(50)
    p = Pair()
    q = S.bow_of(rng, edge_words(rng, 257, NWORDS))
    qwords = sorted(q)
    real = {0, 1, 107, 108, 4095, 8191, 8192, 8193, 8250, 8298, 8299}
    for k in range(8300):
        if k in real:
            bow = S.bow_of(rng, np.concatenate([rng.choice(qwords, 40, replace=False), rng.choice(NWORDS, 200)]))
        elif k % 2:
            bow = {int(qwords[k % len(qwords)] if k % 4 == 1 else rng.integers(NWORDS)): 1.0}
        else:
            bow = {}
        p.dev.add(bow); p.ref.add(bow)
    assert p.dev.size() == (8300, 8300)
    for s in (2, 8191, 8194, 8297):
        p.erase(s)
    common, first, score = p.check_query(q, "8,300 slots")
    assert (common[[8192, 8193, 8250, 8298, 8299]] >= 40).all() and common[8194] == -1 and common[8297] == -1 and common[8191] == -1
    assert (common[8195:8297:2] >= 0).all() and (common[8200:8297] > 0).any()
    slots = [8299, 8192, 0, 8250, 1, 8193, 8298, 8299] + list(range(8195, 8297, 3))
    assert S.same_bits(p.dev.score(q, slots), score[slots])
