"""The descriptor-set operations (vocabulary descent and BowVector, distinctive descriptor, candidate-list matcher, Hamming
matrix) on the CPU: the plain numpy reference (tests/descriptor_sets_reference.py, written from the reference's sources) against
the CPU oracle on every scene of tests/descriptor_sets_scenes.py; what the scenes are FOR, asserted on the reference alone; and
the usual mistakes, each restated here as a deliberately wrong variant that the scenes must tell from the truth.  The same
scenes then run on the device in tests/test_gpu_descriptor_sets.py."""
import functools
import itertools

import numpy as np
import pytest

import oracle
from orb_slam2_e_amd.vocabulary import assemble_bow

import descriptor_sets_reference as ref
import descriptor_sets_scenes as scenes

INT_MAX = ref.INT_MAX
TREES = {s.name: s for s in scenes.tree_scenes()}
WIDE = ("16x17", "17x20", "33x2", "20x20x3")
PAIRS = list(itertools.product(range(6), range(4)))          # ScoringType x WeightingType


def descent(name, levelsup):
    """(word, node, weight, trace) of the numpy reference; computed once, never modified."""
    return ref.descent_of(TREES[name], levelsup)


@functools.lru_cache(maxsize=None)
def distinctive_truth():
    desc, off, where = scenes.distinctive_batch()
    best = ref.distinctive(desc, off)
    best.setflags(write=False)
    return desc, off, where, best


# ------------------------------------------------------------------------------------------------- reference == oracle
@pytest.mark.parametrize("name", list(TREES))
def test_descent_reference_equals_oracle(name):
    s = TREES[name]
    for levelsup in s.levelsups:
        got = descent(name, levelsup)[:3]
        want = oracle.bow_descend(*s.tree, s.features, levelsup)
        for g, w, what in zip(got, want, ("word", "node", "weight")):
            assert np.array_equal(g, w), f"{name}, levelsup {levelsup}: {what}"


def test_distinctive_reference_equals_oracle():
    desc, off, where, best = distinctive_truth()
    assert np.array_equal(best, oracle.distinctive_descriptors(desc, off))
    for desc, off, _ in scenes.distinctive_placements():
        assert np.array_equal(ref.distinctive(desc, off), oracle.distinctive_descriptors(desc, off))


def test_candidates_reference_equals_oracle():
    for A, B, off, idx, _ in scenes.candidate_scenes():
        got = ref.match_candidates(A, B, off, idx)
        want = oracle.match_candidates(A, B, off, idx)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_hamming_reference_equals_oracle():
    for A, B in scenes.hamming_scenes():
        assert np.array_equal(ref.hamming(A, B), oracle.hamming_matrix(A, B))


# ------------------------------------------------------------------------------------------------- BowVector assembly
@pytest.mark.parametrize("name", ["20x20x3", "irregular"])
def test_bow_vector_restatement_equals_assemble_bow_and_fsum(name):
    """assemble_bow (the product's host half) against the second, differently written restatement, value for value, for the 6
    scorings x 4 weightings; and every value against the same quantity with correctly rounded sums.  Bound: n * 2^-52 relative
    for a frame of n features -- a sequential sum of n positive doubles is within (n - 1) * 2^-53 of the exact one, and a value
    is one such sum divided by another (for L2_NORM the root halves the norm's share)."""
    s = TREES[name]
    word, node, _, _ = descent(name, 1)
    n = len(word)
    assert len(np.unique(word)) < n                                  # words seen more than once: addWeight != addIfNotExist
    for scoring, weighting in PAIRS:
        w = s.with_weighting(weighting)[4][np.nonzero(s.tree[3] >= 0)[0]][word]       # the word's weight in that vocabulary
        assert (w == 0).any() and (w > 0).any()                      # stopped words among them
        bow, fv = ref.bow_vector(word, node, w, scoring, weighting)
        gb, gf = assemble_bow(word, node, w, scoring, weighting)
        assert gb == bow and gf == fv, (scoring, weighting)
        assert all(v == sorted(v) and len(v) > 0 for v in fv.values())
        hp = ref.bow_vector_fsum(word, w, scoring, weighting)
        assert hp.keys() == bow.keys()
        for k, x in bow.items():
            assert abs(x - hp[k]) <= n * 2.0 ** -52 * hp[k], (scoring, weighting, k)
    # the outside facts: unit L1 / L2 norm, DOT_PRODUCT's division, first value kept by addIfNotExist
    w = s.tree[4][np.nonzero(s.tree[3] >= 0)[0]][word]
    l1 = ref.bow_vector(word, node, w, ref.L1_NORM, ref.TF_IDF)[0]
    l2 = ref.bow_vector(word, node, w, ref.L2_NORM, ref.TF_IDF)[0]
    dot = ref.bow_vector(word, node, w, ref.DOT_PRODUCT, ref.TF_IDF)[0]
    idf = ref.bow_vector(word, node, w, ref.DOT_PRODUCT, ref.IDF)[0]
    assert abs(sum(l1.values()) - 1.0) < 1e-12 and abs(sum(x * x for x in l2.values()) - 1.0) < 1e-12
    raw = {}
    for i in range(n):
        if w[i] > 0:
            raw[int(word[i])] = raw.get(int(word[i]), 0.0) + w[i]
    assert all(dot[k] == raw[k] / len(raw) for k in raw)
    assert all(idf[int(word[i])] == w[i] for i in range(n) if w[i] > 0)


# ------------------------------------------------------------------------------------------------- the scenes' conditions
@pytest.mark.parametrize("name", WIDE)
def test_wide_trees_use_every_position_and_the_second_chunk(name):
    s = TREES[name]
    off, ids = s.tree[0], s.tree[1]
    trace = descent(name, 0)[3]
    widths = [int(x) for x in name.split("x")]
    assert all(len(p) == len(widths) for p in trace)                 # every leaf at depth L
    for level, k in enumerate(widths):
        assert {p[level] for p in trace} == set(range(k)), f"{name}: level {level + 1}"
    beyond = sum(1 for p in trace if max(p) >= 16)
    assert beyond > 0.05 * len(trace), f"{name}: {beyond} of {len(trace)} descents pass a position >= 16"
    # a leaf is found from its own descriptor, unless it stands behind (or below) a planted equal sibling
    word = descent(name, 0)[0]
    leaves = np.nonzero(s.tree[3] >= 0)[0]
    assert (word[:len(leaves)] == s.tree[3][leaves]).mean() > 0.9


@pytest.mark.parametrize("name", list(TREES))
def test_planted_siblings_are_ties_and_the_first_wins(name):
    s = TREES[name]
    off, ids, desc = s.tree[:3]
    trace = descent(name, 0)[3]
    assert len(s.ties) >= 3 or name == "16x17"
    for f, level, p, q in s.ties:
        assert trace[f][level - 1] == p, f"{name}: feature {f}"
        node = 0
        for pos in trace[f][:level - 1]:
            node = ids[off[node] + pos]
        d = ref.hamming(s.features[f][None], desc[ids[off[node]:off[node + 1]]])[0]
        assert d[p] == d[q] == d.min() and (d == d.min()).sum() == 2 and p < q
    for f, level in s.all256:
        node = 0
        for pos in trace[f][:level - 1]:
            node = ids[off[node] + pos]
        d = ref.hamming(s.features[f][None], desc[ids[off[node]:off[node + 1]]])[0]
        assert len(d) <= 16 and (d == 256).all() and trace[f][level - 1] == 0
    pairs = {(p, q) for _, _, p, q in s.ties}
    assert any((q - p) % 16 == 0 for p, q in pairs) and (15, 16) in pairs     # the same lane of a row in two chunks; the chunk's seam
    assert name == "16x17" or (2, 17) in pairs                                # (no node of that tree has 18 children)
    assert name in ("16x17", "17x20") or s.all256                             # (no one-chunk node below the root in those two)


def test_irregular_tree_has_the_widths_and_depths():
    s = TREES["irregular"]
    off = s.tree[0]
    nchild = set(np.diff(off).tolist())
    assert {1, 15, 16, 17, 31, 32, 33, 48} <= nchild
    trace = descent("irregular", 0)[3]
    depth = np.array([len(p) for p in trace])
    assert set(depth.tolist()) == {1, 2, 3}
    # the four features of a wave (16 lanes each) end at different levels in most waves
    waves = depth[:len(depth) // 4 * 4].reshape(-1, 4)
    assert (waves.min(1) != waves.max(1)).mean() > 0.5
    # a leaf above level L - levelsup keeps node id 0
    node = descent("irregular", 0)[1]
    assert (node[depth < 3] == 0).all() and (node[depth == 3] > 0).all()


def test_distinctive_groups_meet_their_purpose():
    desc, off, where, best = distinctive_truth()
    groups = scenes.distinctive_groups()
    assert [len(g) for _, g, _ in groups[:len(scenes.DD_SIZES)]] == list(scenes.DD_SIZES)
    residues = set()
    for (name, g, want), at in zip(groups, where):
        assert off[at + 1] - off[at] == len(g) and off[at + 2] == off[at + 1]       # an empty point after each
        if want is not None:
            assert best[at] == want, name
        if len(g) > 128:
            residues.add(int(ref.distinctive_medians(g)[best[at]]) % 5)
    assert residues == {0, 1, 2, 3, 4}
    assert (best[1::2] == -1).all()
    named = {n: g for n, g, _ in groups}
    assert list(ref.distinctive_medians(named["a and three complements"])) == [256, 0, 0, 0]
    r65 = int(best[where[[n for n, _, _ in groups].index("random 65")]])
    for desc, off, pos in scenes.distinctive_placements():                           # the same answers wherever the points stand
        assert list(ref.distinctive(desc, off)[pos]) == [64, r65, 128]


def test_candidate_and_hamming_scenes_meet_their_purpose():
    seen = set()
    sizes = set()
    for A, B, off, idx, planted in scenes.candidate_scenes():
        best, second, arg = ref.match_candidates(A, B, off, idx)
        sizes.add(len(A))
        seen |= set(np.diff(off).tolist())
        for i, kind in planted.items():
            if kind == "twice":
                assert off[i + 1] - off[i] == 2 and idx[off[i]] == idx[off[i] + 1] and second[i] == best[i] < INT_MAX
            elif kind == "equal pair":
                assert idx[off[i]] != idx[off[i] + 1] and arg[i] == idx[off[i]] and second[i] == best[i]
            else:
                assert (best[i], second[i], arg[i]) == (256, INT_MAX, idx[off[i]])
        empty = np.diff(off) == 0
        assert (best[empty] == INT_MAX).all() and (second[empty] == INT_MAX).all() and (arg[empty] == -1).all()
        if len(B) == 0:
            assert empty.all()
    assert sizes == {1, 5, 255, 256, 257} and seen == {0, 1, 2, 40}
    assert [(len(A), len(B)) for A, B in scenes.hamming_scenes()] == list(scenes.HAMMING_SHAPES)
    for A, B in scenes.hamming_scenes():
        D = ref.hamming(A, B)
        assert (D == 256).any() and (D.size == 1 or (D == 0).any())


def test_counts_beyond_the_grid_y_limit_are_refused_before_the_device_is_touched():
    """orbm_match_batch_dev (npairs) and orbm_bow_transform_batch_dev (nsets) above ORBM_MAX_GRID_Y = 65,535: ORBX_ERR_UNSUPPORTED with
    the limit in the message, decided on the host before any device call -- so it shows on a machine without a GPU as well (the
    device tests check that nothing was queued)."""
    from orb_slam2_e_amd._lib import lib, ptr
    L = lib()
    a = np.zeros(64, np.int32)
    assert L.orbm_match_batch_dev(ptr(a), ptr(a), 1, None, None, 65536, 50, 0.6, None, None, None, None, None, None) == -5
    assert b"65,535 pairs" in L.orbx_last_error()
    assert L.orbm_bow_transform_batch_dev(ptr(a), ptr(a), ptr(a), 1, 65536, 0, ptr(a), ptr(a), None) == -5
    assert b"65,535 descriptor sets" in L.orbx_last_error()
    from orb_slam2_e_amd._lib import HEADERS
    with open(HEADERS[0]) as f:
        assert "#define ORBM_MAX_GRID_Y 65535" in f.read()


# ------------------------------------------------------------------------------------------------- the usual mistakes
def _descend(tree, features, levelsup, pick, nid_shift=0, nid_at_leaf=False):
    """The descent with its decisions pulled out: pick(d) -> position; the node id taken at level L - levelsup + nid_shift."""
    child_off, child_ids, node_desc, node_word, _, L = tree
    word, node = [], []
    for f in features:
        final_id, level, nid = 0, 0, 0
        while True:
            level += 1
            kids = child_ids[child_off[final_id]:child_off[final_id + 1]]
            final_id = int(kids[pick(np.unpackbits(f[None, :] ^ node_desc[kids], axis=1).sum(axis=1))])
            if level == L - levelsup + nid_shift:
                nid = final_id
            if child_off[final_id + 1] == child_off[final_id]:
                break
        if nid_at_leaf and level < L - levelsup:
            nid = final_id
        word.append(node_word[final_id]); node.append(nid)
    return np.array(word, np.int32), np.array(node, np.int32)


_first = lambda d: int(np.argmin(d))
DESCENT_MISTAKES = {
    "only the first 16 children": dict(pick=lambda d: int(np.argmin(d[:16]))),
    "last closest child wins": dict(pick=lambda d: len(d) - 1 - int(np.argmin(d[::-1]))),
    "tie between p and p + 16 goes to p + 16": dict(pick=lambda d: min(range(len(d)), key=lambda p: (d[p], p & 15, -p))),
    "node id one level early": dict(pick=_first, nid_shift=-1),
    "node id one level late": dict(pick=_first, nid_shift=1),
    "node id left at an early leaf": dict(pick=_first, nid_at_leaf=True),
}


def test_descent_restated_with_hooks_is_the_reference():
    for name, s in TREES.items():
        for levelsup in s.levelsups:
            word, node = _descend(s.tree, s.features, levelsup, _first)
            assert np.array_equal(word, descent(name, levelsup)[0]) and np.array_equal(node, descent(name, levelsup)[1])


@pytest.mark.parametrize("mistake", list(DESCENT_MISTAKES))
def test_scenes_tell_descent_mistakes_apart(mistake):
    told = []
    for name, s in TREES.items():
        for levelsup in s.levelsups:
            word, node = _descend(s.tree, s.features, levelsup, **DESCENT_MISTAKES[mistake])
            if not (np.array_equal(word, descent(name, levelsup)[0]) and np.array_equal(node, descent(name, levelsup)[1])):
                told.append((name, levelsup))
    assert told, mistake
    if mistake in ("only the first 16 children", "last closest child wins", "tie between p and p + 16 goes to p + 16"):
        assert {n for n, _ in told} == set(TREES), told              # every tree on its own
    if "tie" in mistake or "last" in mistake:                        # ... and every planted tie on its own
        for name, s in TREES.items():
            word, _ = _descend(s.tree, s.features[[f for f, *_ in s.ties]], 0, DESCENT_MISTAKES[mistake]["pick"])
            truth = descent(name, 0)[0][[f for f, *_ in s.ties]]
            for (f, level, p, q), w, t in zip(s.ties, word, truth):
                if "last" in mistake or (q - p) % 16 == 0:
                    assert w != t, (name, f)


_MATRICES = {}


def _matrix(d):
    """The N x N distances of one point's rows: computed once per group, whichever variant asks."""
    key = d.tobytes()
    if key not in _MATRICES:
        _MATRICES[key] = ref.hamming(d, d)
        _MATRICES[key].setflags(write=False)
    return _MATRICES[key]


def _distinctive(desc, off, mistake=None):
    """(best, medians of every row) with one decision changed."""
    best, meds = np.full(len(off) - 1, -1, np.int32), []
    for i in range(len(off) - 1):
        d = desc[off[i]:off[i + 1]]
        N = len(d)
        if N == 0:
            continue
        D = _matrix(d).copy()
        np.fill_diagonal(D, 0)
        if mistake == "distances capped at 255":
            D = np.minimum(D, 255)
        if mistake == "diagonal left out":
            rows = np.sort(D[~np.eye(N, dtype=bool)].reshape(N, N - 1), axis=1)
            med = rows[:, min(int(0.5 * (N - 1)), N - 2)] if N > 1 else np.zeros(1, np.int32)
        else:
            med = np.sort(D, axis=1)[:, N // 2 if mistake == "median index N // 2" else int(0.5 * (N - 1))]
        if mistake == "rows past 127 ignored":
            med = med[:128]
        best[i] = len(med) - 1 - int(np.argmin(med[::-1])) if mistake == "last row wins ties" else int(np.argmin(med))
        meds.append(med)
    return best, meds


@pytest.mark.parametrize("mistake", ["median index N // 2", "diagonal left out", "last row wins ties", "rows past 127 ignored"])
def test_scenes_tell_distinctive_mistakes_apart(mistake):
    desc, off, where, best = distinctive_truth()
    assert np.array_equal(_distinctive(desc, off)[0], best)
    got = _distinctive(desc, off, mistake)[0]
    differ = [scenes.distinctive_groups()[where.index(i)][0] for i in np.nonzero(got != best)[0]]
    assert differ, mistake
    if mistake == "rows past 127 ignored":
        assert {"planted row 128 of 129", "planted row 699 of 700"} <= set(differ)
    if mistake == "last row wins ties":
        assert {"200 identical rows", "two equal winners, short path", "two equal winners, long path"} <= set(differ)


def test_a_distance_cap_of_255_shows_in_the_medians_only():
    """A row's median can be 256 only if more than half of the rows are the row's complement; those rows are then equal to each
    other and have median 0, so a row with median 256 never wins and never ties: no group exists on which min(d, 255) changes the
    WINNER.  The cap is therefore told apart where it can be: in the row medians of {a, ~a, ~a, ~a} here, and in the Hamming
    matrix and the candidate lists (best = 256 for a complement), which the device tests compare entry by entry."""
    named = {n: g for n, g, _ in scenes.distinctive_groups()}
    g = named["a and three complements"]
    off = np.array([0, 4], np.int32)
    true_best, true_med = _distinctive(g, off)
    cap_best, cap_med = _distinctive(g, off, "distances capped at 255")
    assert list(true_med[0]) == [256, 0, 0, 0] and list(cap_med[0]) == [255, 0, 0, 0] and true_best[0] == cap_best[0] == 1
    capped = lambda A, B: np.minimum(ref.hamming(A, B), 255)
    assert any(not np.array_equal(capped(A, B), ref.hamming(A, B)) for A, B in scenes.hamming_scenes())
    A, B, off, idx, planted = scenes.candidate_scenes()[4]
    i = [q for q, kind in planted.items() if kind == "complement"][0]
    assert ref.match_candidates(A, B, off, idx)[0][i] == 256


def _candidates(A, B, off, idx, mistake):
    nA = len(A)
    best = np.zeros(nA, np.int32); second = np.zeros(nA, np.int32); arg = np.zeros(nA, np.int32)
    for i in range(nA):
        b, s, a = (0, 0, 0) if mistake == "zeros for an empty list" and off[i] == off[i + 1] else (INT_MAX, INT_MAX, -1)
        for k in range(off[i], off[i + 1]):
            j = int(idx[k])
            d = int(ref.hamming(A[i][None], B[j][None])[0, 0])
            if d < b or (mistake == "<= in the first compare" and d == b):
                s, b, a = b, d, j
            elif d < s and not (mistake == "second not updated by an equal distance" and d == b):
                s = d
        best[i], second[i], arg[i] = b, s, a
    return best, second, arg


@pytest.mark.parametrize("mistake", ["<= in the first compare", "second not updated by an equal distance", "zeros for an empty list"])
def test_scenes_tell_candidate_mistakes_apart(mistake):
    differ = 0
    for A, B, off, idx, planted in scenes.candidate_scenes():
        truth = ref.match_candidates(A, B, off, idx)
        assert all(np.array_equal(g, t) for g, t in zip(_candidates(A, B, off, idx, None), truth))
        got = _candidates(A, B, off, idx, mistake)
        differ += any(not np.array_equal(g, t) for g, t in zip(got, truth))
        if mistake == "<= in the first compare":
            for i, kind in planted.items():
                if kind == "equal pair":
                    assert got[2][i] != truth[2][i]
    assert differ >= 4, mistake
