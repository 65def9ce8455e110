"""The keyframe database (orbm_kfdb_*, orb_slam2_e_amd/keyframe_database.py), the part that needs no device: the two restatements
of src/KeyFrameDatabase.cc (tests/kfdb_reference.py, tests/kfdb_oracle.cc) agree bit for bit; hand-built cases with known answers;
stages 2 and 3 of the host class, fed the restatement's counts, give the restatement's candidates and persistent fields; and the
new entry points are declared, exported and bound, and refuse bad arguments before they ask for a device.

orbm_kfdb_add uploads the row, so an ACCEPTED add, and with it the refusals that need a resident row (erase of a dead slot, a second
erase, a dead slot in score's list), need a device: tests/test_gpu_kfdb.py has those."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import kfdb_reference as R
import kfdb_scenes as S
from orb_slam2_e_amd import keyframe_database as K
from orb_slam2_e_amd._lib import lib, prototypes
from test_cpu_integration_shells import _calls, _declarations, _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -2
F32 = np.float32
NO_GRAPH = lambda slot: []


@pytest.fixture(scope="module")
def oracle_exe(tmp_path_factory):
    return S.build_oracle(tmp_path_factory.mktemp("kfdb"))


def flat(words):
    """a BowVector with the same value on every word"""
    return S.normalised(list(words), [1.0] * len(words))


class HostOverCounts:
    """Stages 2 and 3 of the host class over (common, first, score) taken from the restatement's counting (a ReferenceDatabase of
    its own, of which only add / erase / clear / shared are used: no field of it is ever written)."""
    def __init__(self, nwords):
        self.counts = R.ReferenceDatabase(nwords)
        self.fields = K.SlotFields()

    def add(self, bow):
        s = self.counts.add(bow)
        self.fields.resize(s + 1)
        return s

    def erase(self, slot):
        self.counts.erase(slot)

    def clear(self):
        self.counts.clear()
        self.fields.resize(0)

    def detect_loop_candidates(self, bow, qid, connected, min_score, best):
        scored, min_common = K.loop_stage2(self.fields, *self.counts.shared(bow), qid, connected, min_score)
        return K.loop_stage3(self.fields, scored, min_common, qid, min_score, best)

    def detect_relocalization_candidates(self, bow, qid, best):
        scored, _ = K.reloc_stage2(self.fields, *self.counts.shared(bow), qid)
        return K.reloc_stage3(self.fields, scored, qid, best)


def same_fields(got, want, what):
    for name, g, w in zip(K.SlotFields.NAMES, got, want):
        if g.dtype == np.float32:
            assert S.same_bits(g, w), f"{what}: {name}"
        else:
            assert np.array_equal(g, w), f"{what}: {name}: {g} != {w}"


def play(db, ops):
    """runs sequence() operations on a database with the host class's methods; per query (candidates, fields after it)"""
    graph, out = {}, []
    best = lambda s: graph.get(s, [])
    for op in ops:
        if op[0] == "add":
            graph[db.add(op[1])] = op[2] if len(op) > 2 else []
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear(); graph.clear()
        elif op[0] == "loop":
            out.append((db.detect_loop_candidates(op[1], op[2], op[3], op[4], best), [a.copy() for a in _fields(db)]))
        elif op[0] == "reloc":
            out.append((db.detect_relocalization_candidates(op[1], op[2], best), [a.copy() for a in _fields(db)]))
    return out


def _fields(db):
    return db.fields() if isinstance(db, R.ReferenceDatabase) else db.fields.arrays()


SEQUENCES = [dict(seed=1), dict(seed=2, nkf=64, nqueries=10, words=80), dict(seed=3, clear_at=3), dict(seed=4, nplaces=1, nkf=30, nqueries=6),
             dict(seed=5, nwords=200, words=90, nkf=48)]


# ------------------------------------------------------------------------------------------------ the two restatements agree
@pytest.mark.parametrize("kw", SEQUENCES, ids=lambda kw: "seed%d" % kw["seed"])
def test_python_and_cxx_restatements_agree(kw, oracle_exe):
    """counts, list order, scores, both candidate lists and the six fields after every query of a sequence"""
    nwords = kw.get("nwords", 1000)
    ops = S.sequence(**kw)
    probes = []
    for op in ops:                                   # in front of every query: what it will find, and a score list
        if op[0] in ("loop", "reloc"):
            probes += [("shared", op[1]), ("score*", op[1])]
        probes.append(op)
    ref = R.ReferenceDatabase(nwords)
    graph, want, text_ops = {}, [], []
    best = lambda s: graph.get(s, [])
    for op in probes:
        if op[0] == "add":
            graph[ref.add(op[1])] = op[2]
        elif op[0] == "erase":
            ref.erase(op[1])
        elif op[0] == "clear":
            ref.clear(); graph.clear()
        elif op[0] == "shared":
            want.append(("Q",) + ref.shared(op[1]))
        elif op[0] == "score*":
            live = [k.slot for k in ref.kfs if k.alive]
            slots = (live + live[:3])[:25]                                 # some slots twice
            op = ("score", op[1], slots)
            want.append(("S", ref.score(op[1], slots)))
        elif op[0] == "loop":
            c = ref.detect_loop_candidates(op[1], op[2], op[3], op[4], best)
            want += [("L", c, ref.last_sharing), ("F", ref.fields())]
        elif op[0] == "reloc":
            c = ref.detect_relocalization_candidates(op[1], op[2], best)
            want += [("R", c, ref.last_sharing), ("F", ref.fields())]
        text_ops.append(op)
    got = [r for r in S.run_oracle(oracle_exe, S.case_text(nwords, text_ops)) if r[0] != "A"]
    assert [r[0] for r in got] == [r[0] for r in want]
    ncand = 0
    for g, w in zip(got, want):
        if g[0] == "Q":
            assert np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]) and S.same_bits(g[3], w[3])
        elif g[0] == "S":
            assert S.same_bits(g[1], w[1])
        elif g[0] == "F":
            same_fields(g[1], w[1], "fields")
        else:
            assert g[1] == w[1] and g[2] == w[2], (g, w)
            ncand += len(g[1])
    assert ncand > 0                                 # the scenes do produce candidates


@pytest.mark.parametrize("kw", SEQUENCES, ids=lambda kw: "seed%d" % kw["seed"])
def test_host_stages_give_the_restatements_candidates_and_fields(kw):
    """at least five queries with adds and erases in between, the host stages fed the restatement's counts"""
    ops = S.sequence(**kw)
    assert sum(op[0] in ("loop", "reloc") for op in ops) >= 5 and any(op[0] == "erase" for op in ops)
    want = play(R.ReferenceDatabase(kw.get("nwords", 1000)), ops)
    got = play(HostOverCounts(kw.get("nwords", 1000)), ops)
    for i, ((gc, gf), (wc, wf)) in enumerate(zip(got, want)):
        assert gc == wc, f"query {i}: candidates"
        same_fields(gf, wf, f"query {i}")


def test_sharing_order_is_first_shared_word_then_slot():
    ref = R.ReferenceDatabase(100)
    for words in ([40, 50], [10, 50], [40, 60], [10, 20], [90]):
        ref.add(flat(words))
    q = flat([10, 40, 50, 60])
    ref.detect_relocalization_candidates(q, 1, NO_GRAPH)
    assert ref.last_sharing == [1, 3, 0, 2]
    common, first, _ = ref.shared(q)
    assert list(K.sharing_order(common, first)) == [1, 3, 0, 2] and list(first) == [1, 0, 1, 0, -1] and list(common) == [2, 2, 2, 1, 0]


# ------------------------------------------------------------------------------------------------ known answers
def both(nwords=100):
    return R.ReferenceDatabase(nwords), HostOverCounts(nwords)


def test_scores_of_identical_disjoint_and_one_shared_word():
    ref = R.ReferenceDatabase(100)
    a = {1: 0.25, 5: 0.25, 7: 0.5}
    ref.add(a); ref.add({2: 0.5, 9: 0.5}); ref.add({3: 0.5, 9: 0.5})
    s = ref.score(a, [0, 1])
    assert abs(float(s[0]) - 1.0) < 1e-6 and s[1] == 0.0 and np.signbit(s[1])           # identical: 1.0; disjoint: -0.0
    assert ref.score({3: 1.0}, [2])[0] == F32(0.5)                                       # |1 - .5| - 1 - .5 = -1, -(-1) / 2
    common, first, score = ref.shared(a)
    assert list(common) == [3, 0, 0] and list(first) == [0, -1, -1] and np.signbit(score[1]) and np.signbit(score[2])
    rng = np.random.default_rng(0)
    b = S.bow_of(rng, rng.choice(1000, 300, replace=False))
    assert abs(float(R.l1_score(sorted(b), [b[w] for w in sorted(b)], sorted(b), [b[w] for w in sorted(b)])) - 1.0) < 1e-12


def test_count_equal_to_min_common_words_is_excluded():
    """max = 5 -> minCommonWords = int(5 * 0.8f) = 4; the comparison is strict: a keyframe sharing 4 words is not scored"""
    assert R.min_common_words(5) == 4
    for db in both():
        db.add(flat([1, 2, 3, 4, 5])); db.add(flat([1, 2, 3, 4, 50])); db.add(flat([1, 2, 3, 51, 52]))
        assert db.detect_relocalization_candidates(flat([1, 2, 3, 4, 5]), 3, NO_GRAPH) == [0]
        f = _fields(db)
        assert list(f[3]) == [3, 3, 3] and list(f[4]) == [5, 4, 3] and f[5][0] > 0 and f[5][1] == 0 and f[5][2] == 0
        # one more shared word and it is scored
    for db in both():
        db.add(flat([1, 2, 3, 4, 5, 6])); db.add(flat([1, 2, 3, 4, 5, 50]))
        assert R.min_common_words(6) == 4
        db.detect_relocalization_candidates(flat([1, 2, 3, 4, 5, 6]), 3, NO_GRAPH)
        assert _fields(db)[5][1] > 0


def test_float_and_double_cut_agree_below_8192():
    """int(max * 0.8f) in float against floor(max * 0.8) in double: the search finds NO maxCommonWords up to 8,192 (a BowVector's
    limit here) at which they differ -- 0.8f and 0.8 both lie above 4/5, multiples of 5 round to the integer itself in either
    format, and every other product is at least 0.2 away from an integer -- so there is no such case to build.  What IS pinned is
    the float form, on all of them."""
    differ = [m for m in range(1, 8193) if int(F32(m) * F32(0.8)) != math.floor(m * 0.8)]
    assert differ == []
    assert all(R.min_common_words(m) == K.min_common_words(m) == (4 * m) // 5 for m in range(1, 8193))


def test_query_id_zero_lists_nobody():
    for db in both():
        db.add(flat([1, 2, 3])); db.add(flat([2, 3, 4]))
        assert db.detect_relocalization_candidates(flat([1, 2, 3]), 0, NO_GRAPH) == []
        assert db.detect_loop_candidates(flat([1, 2, 3]), 0, [], 0.0, NO_GRAPH) == []
        f = _fields(db)
        assert list(f[0]) == [0, 0] and list(f[1]) == [3, 2] and list(f[3]) == [0, 0] and list(f[4]) == [3, 2]     # counted on, never listed
        assert list(f[2]) == [0, 0] and list(f[5]) == [0, 0]
    ref = R.ReferenceDatabase(100)
    ref.add(flat([1])); ref.detect_loop_candidates(flat([1]), 0, [], 0.0, NO_GRAPH)
    assert ref.last_sharing == []


def test_tie_in_accumulated_score_keeps_list_order():
    """two keyframes with the same BowVector, each the other's neighbour: both accumulate s + s, neither replaces the other as best
    (the comparison is strict), and the candidates come in list order; in the second scene slot 1 comes first, because its first
    shared word is the earlier one in the query"""
    for db in both():
        db.add(flat([5, 6, 7])); db.add(flat([5, 6, 7])); db.add(flat([4, 5, 6, 7]))
        graph = {0: [1], 1: [0], 2: []}
        assert db.detect_loop_candidates(flat([5, 6, 7]), 9, [2], 0.0, lambda s: graph[s]) == [0, 1]
        f = _fields(db)
        assert f[2][0] == f[2][1] and f[2][0] > F32(0.99)
    for db in both():
        db.add(flat([5, 6, 7])); db.add(flat([4, 5, 6]))
        assert db.detect_relocalization_candidates(flat([4, 5, 6, 7]), 9, NO_GRAPH) == [1, 0]


def test_stale_reloc_score_of_an_unscored_neighbour_enters_the_sum():
    """query 5 scores B high.  Query 6 lists B (one shared word) but the word cut drops it, so mRelocScore of B is still query 5's;
    A's neighbour B passes `mnRelocQuery == id`, its stale score is added and, being larger, makes B the candidate."""
    for db in both():
        a = db.add(flat([1, 2, 3, 4, 5, 30, 31, 32, 33, 34])); b = db.add(flat([5, 20, 21, 22, 23]))
        assert db.detect_relocalization_candidates(flat([5, 20, 21, 22, 23]), 5, NO_GRAPH) == [b]
        stale = _fields(db)[5][b]
        assert stale > F32(0.99)
        graph = {a: [b], b: []}
        assert db.detect_relocalization_candidates(flat([1, 2, 3, 4, 5]), 6, lambda s: graph[s]) == [b]
        f = _fields(db)
        assert list(f[3]) == [6, 6] and list(f[4]) == [5, 1] and f[5][b] == stale and F32(0) < f[5][a] < stale
        # without the neighbour: A itself
        assert db.detect_relocalization_candidates(flat([1, 2, 3, 4, 5]), 7, NO_GRAPH) == [a]


def test_connected_keyframe_with_most_words_does_not_raise_the_maximum():
    for connected, want in (([], [0]), ([0], [1])):
        for db in both():
            db.add(flat(range(1, 11))); db.add(flat([1, 2, 3, 4, 5, 40])); db.add(flat([1, 2, 3, 4, 41]))
            assert db.detect_loop_candidates(flat(range(1, 11)), 4, connected, 0.0, NO_GRAPH) == want
            f = _fields(db)
            if connected:        # max = 5 -> cut 4: slot 1 scored, slot 2 (4 words) not; the connected one: never listed, words left at 1
                assert list(f[0]) == [0, 4, 4] and list(f[1]) == [1, 5, 4] and f[2][0] == 0 and f[2][1] > 0 and f[2][2] == 0
            else:                # max = 10 -> cut 8: only slot 0
                assert list(f[0]) == [4, 4, 4] and list(f[1]) == [10, 5, 4] and f[2][1] == 0


def test_min_score_filter_and_repeated_query_id():
    for db in both():
        db.add(flat([1, 2, 3, 4, 5, 6])); db.add(flat([1, 2, 3, 4, 5, 50]))
        q = flat([1, 2, 3, 4, 5, 6])
        assert db.detect_loop_candidates(q, 8, [], 0.9, NO_GRAPH) == [0]          # slot 1 scores 5/6 < 0.9: scored, field written, dropped
        f = _fields(db)
        assert abs(float(f[2][1]) - 5 / 6) < 1e-6 and list(f[1]) == [6, 5]
        assert db.detect_loop_candidates(q, 8, [], 0.0, NO_GRAPH) == []           # same id again: nobody is listed, the counts run on
        assert list(_fields(db)[1]) == [12, 10]


def test_erase_keeps_the_order_of_the_others_and_clear_restarts_slots():
    for db in both():
        for _ in range(4):
            db.add(flat([7, 8]))
        db.erase(1)
        assert db.detect_relocalization_candidates(flat([7, 8]), 2, NO_GRAPH) == [0, 2, 3]
        assert list(_fields(db)[3]) == [2, 0, 2, 2]
        db.clear()
        assert db.add(flat([8, 9])) == 0
        assert db.detect_relocalization_candidates(flat([7, 8]), 2, NO_GRAPH) == [0]
        assert [len(a) for a in _fields(db)] == [1] * 6 and _fields(db)[4][0] == 1
    ref = R.ReferenceDatabase(100)
    for _ in range(3):
        ref.add(flat([7]))
    ref.erase(1)
    common, first, score = ref.shared(flat([7]))
    assert list(common) == [1, -1, 1] and list(first) == [0, -1, 0] and score[1] == 0 and not np.signbit(score[1])


# ------------------------------------------------------------------------------------------------ the C ABI without a device
NEW = {"orbm_kfdb_create": 2, "orbm_kfdb_destroy": 1, "orbm_kfdb_add": 5, "orbm_kfdb_erase": 2, "orbm_kfdb_clear": 1, "orbm_kfdb_size": 3,
       "orbm_kfdb_query": 7, "orbm_kfdb_score": 7, "orbm_debug_last_kfdb_waits": 0, "orbm_debug_kfdb_reallocs": 1,
       "orbm_debug_kfdb_max_blocks": 1}


def test_new_symbols_are_declared_exported_and_bound():
    protos = prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_kfdb_create"] == (i, [i, vp]) and protos["orbm_kfdb_add"] == (i, [vp, vp, vp, i, vp])
    assert protos["orbm_kfdb_erase"] == (i, [vp, i]) and protos["orbm_kfdb_size"] == (i, [vp, vp, vp])
    assert protos["orbm_kfdb_query"] == (i, [vp, vp, vp, i, vp, vp, vp]) and protos["orbm_kfdb_score"] == (i, [vp, vp, vp, i, vp, i, vp])
    assert protos["orbm_debug_last_kfdb_waits"] == (i, [])
    L = lib()
    assert L.orbx_abi_version() == 136
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name]).decode()
    for name, nargs in NEW.items():
        assert len(protos[name][1]) == nargs and getattr(L, name).argtypes == protos[name][1], name
        assert f" T {name}\n" in out, name
    hpp = open(os.path.join(ROOT, "include", "orbslam_hip.hpp")).read()
    assert "class KeyFrameDatabase" in hpp and "orbm_kfdb_query" in hpp and "orbm_kfdb_score" in hpp
    import orb_slam2_e_amd
    assert orb_slam2_e_amd.KeyFrameDatabase is K.KeyFrameDatabase


def _arr(values, t):
    a = np.array(values, t)
    return a, a.ctypes.data_as(C.c_void_p)


def test_bare_library_accepts_and_refuses_without_a_device():
    import torch
    L = lib()
    assert L.orbm_kfdb_create(0, C.byref(C.c_void_p())) == ERR_ARG and L.orbm_kfdb_create(10, None) == ERR_ARG
    h = C.c_void_p()
    assert L.orbm_kfdb_create(10, C.byref(h)) == 0 and h
    live, slots = C.c_int(-1), C.c_int(-1)
    assert L.orbm_kfdb_size(h, C.byref(live), C.byref(slots)) == 0 and (live.value, slots.value) == (0, 0)
    assert L.orbm_kfdb_size(None, C.byref(live), C.byref(slots)) == ERR_ARG
    assert L.orbm_kfdb_clear(h) == 0 and L.orbm_debug_kfdb_reallocs(h) == 0
    slot = C.c_int(-7)
    ps = C.byref(slot)
    big_w, pbw = _arr(np.arange(8193), np.int32)
    big_v, pbv = _arr(np.full(8193, 1 / 8193), np.float64)
    v, pv = _arr([0.25, 0.25, 0.5], np.float64)
    waits = L.orbm_debug_last_kfdb_waits()
    bad_rows = ([1, 1, 2], [2, 1, 3], [-1, 2, 3], [1, 2, 10])               # equal, descending, below 0, nwords itself
    for ids in bad_rows:
        w, pw = _arr(ids, np.int32)
        assert L.orbm_kfdb_add(h, pw, pv, 3, ps) == ERR_ARG and b"ascending" in L.orbx_last_error(), ids
    w, pw = _arr([1, 2, 9], np.int32)
    assert L.orbm_kfdb_add(h, pw, pv, -1, ps) == ERR_ARG
    assert L.orbm_kfdb_add(h, pbw, pbv, 8193, ps) == ERR_ARG and b"8,192" in L.orbx_last_error()
    assert L.orbm_kfdb_add(h, pw, pv, 3, None) == ERR_ARG and L.orbm_kfdb_add(h, None, pv, 3, ps) == ERR_ARG
    assert L.orbm_kfdb_add(None, pw, pv, 3, ps) == ERR_ARG
    assert slot.value == -7
    for s in (-1, 0, 5):
        assert L.orbm_kfdb_erase(h, s) == ERR_ARG and b"slot" in L.orbx_last_error()
    out3 = [np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, -7, np.float32)]
    pc, pf, psc = (a.ctypes.data_as(C.c_void_p) for a in out3)
    for ids in bad_rows:
        bw, pbad = _arr(ids, np.int32)
        assert L.orbm_kfdb_query(h, pbad, pv, 3, pc, pf, psc) == ERR_ARG
        assert L.orbm_kfdb_score(h, pbad, pv, 3, None, 0, psc) == ERR_ARG
    assert L.orbm_kfdb_query(h, pw, pv, -1, pc, pf, psc) == ERR_ARG and L.orbm_kfdb_query(h, pbw, pbv, 8193, pc, pf, psc) == ERR_ARG
    for outs in ((None, pf, psc), (pc, None, psc), (pc, pf, None)):
        assert L.orbm_kfdb_query(h, pw, pv, 3, *outs) == ERR_ARG
    one, pone = _arr([0], np.int32)
    assert L.orbm_kfdb_score(h, pw, pv, 3, pone, 1, psc) == ERR_ARG and b"slot" in L.orbx_last_error()      # no such slot
    assert L.orbm_kfdb_score(h, pw, pv, 3, pone, -1, psc) == ERR_ARG and L.orbm_kfdb_score(h, pw, pv, 3, pone, 1, None) == ERR_ARG
    assert L.orbm_kfdb_score(h, pw, pv, 3, None, 0, None) == ERR_ARG                                    # a NULL output, also with nothing to score
    assert L.orbm_kfdb_score(h, pw, pv, -1, pone, 0, psc) == ERR_ARG
    assert all((a == -7).all() for a in out3) and L.orbm_debug_last_kfdb_waits() == waits                  # refused calls write nothing
    # a call that launches nothing needs no device: the empty database, an empty query, an empty list
    empty3 = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)]
    assert L.orbm_kfdb_query(h, pw, pv, 3, *(a.ctypes.data_as(C.c_void_p) for a in empty3)) == 0 and L.orbm_debug_last_kfdb_waits() == 0
    assert L.orbm_kfdb_query(h, None, None, 0, *(a.ctypes.data_as(C.c_void_p) for a in empty3)) == 0
    assert L.orbm_kfdb_score(h, pw, pv, 3, None, 0, psc) == 0 and L.orbm_debug_last_kfdb_waits() == 0
    assert L.orbm_debug_kfdb_max_blocks(0) == 0
    # arguments first, then the device: a good add is accepted where there is one
    rc = L.orbm_kfdb_add(h, pw, pv, 3, ps)
    assert rc == (0 if torch.cuda.is_available() else ERR_NO_DEVICE)
    assert L.orbm_kfdb_destroy(h) == 0 and L.orbm_kfdb_destroy(None) == 0


def test_integration_shell_calls_the_declared_entry_points():
    decl, header_text = _declarations()
    src = open(os.path.join(ROOT, "integration", "KeyFrameDatabase_hip.cc")).read()
    called = set()
    for fn, nargs in _calls(src):
        if fn not in decl:
            assert re.search(r"\b%s\b" % fn, header_text), f"{fn} is not in include/*.h"
            continue
        assert decl[fn] == nargs, f"{fn} called with {nargs} arguments, declared with {decl[fn]}"
        assert hasattr(lib(), fn)
        called.add(fn)
    assert called == {"orbm_kfdb_create", "orbm_kfdb_destroy", "orbm_kfdb_add", "orbm_kfdb_erase", "orbm_kfdb_clear", "orbm_kfdb_query", "orbm_kfdb_score", "orbx_last_error"}
    code = _strip_comments(src)
    for tok in set(re.findall(r"\b(?:ORBX|ORBM)_[A-Z0-9_]+\b", code)):
        assert re.search(r"\b%s\b" % tok, header_text), tok
    for method in ("add", "erase", "clear", "DetectLoopCandidates", "DetectRelocalizationCandidates"):
        assert len(re.findall(r"^[\w:<>\* ]*\bKeyFrameDatabase::%s\s*\(" % method, code, re.M)) == 1, method
    assert len(re.findall(r"^bool HipDetectLoopMinScore\(", code, re.M)) == 1 and len(re.findall(r"^void HipKeyFrameDatabaseRelease\(", code, re.M)) == 1
    assert "KfdbCandidatesFromCounts" in code and "maxCommonWords" not in code       # the host logic is the header's, not a copy
    assert "KeyFrameDatabase_hip" not in open(os.path.join(ROOT, "integration", "reference.patch")).read()
    for doc in ("INTEGRATION.md", os.path.join("integration", "README.md")):
        assert "KeyFrameDatabase_hip.cc" in open(os.path.join(ROOT, doc)).read(), doc
