"""GPU: k_bow_transform, k_distinctive, k_match_cands and k_hamming_matrix at their tiling edges and limits, on the scenes of
tests/descriptor_sets_scenes.py (whose purpose tests/test_cpu_descriptor_sets.py asserts).  Every result is compared bit for bit
with the plain numpy reference (tests/descriptor_sets_reference.py) AND with the CPU oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from orb_slam2_e_amd import ORBmatcher
from orb_slam2_e_amd._lib import OrbxError, lib, ptr
from orb_slam2_e_amd.vocabulary import ORBVocabulary

import descriptor_sets_reference as ref
import descriptor_sets_scenes as scenes

ERR_ARG, ERR_UNSUPPORTED = -1, -5
INT_MAX = ref.INT_MAX
TREES = {s.name: s for s in scenes.tree_scenes()}


@functools.lru_cache(maxsize=None)
def vocabulary(name, weighting=0):
    return ORBVocabulary(*TREES[name].with_weighting(weighting), scoring=0, weighting=weighting)


# ------------------------------------------------------------------------------------------------------------- descent
@pytest.mark.parametrize("name", list(TREES))
def test_descent_host_arrays(name):
    """orbm_bow_transform on every leaf's descriptor, a noisy copy of each and the planted ties, for levelsup 0, 1, L - 1, L, L + 1."""
    s = TREES[name]
    voc = vocabulary(name)
    for levelsup in s.levelsups:
        got = voc.descend(s.features, levelsup)
        want = ref.descent_of(s, levelsup)[:3]
        orc = oracle.bow_descend(*s.tree, s.features, levelsup)
        for g, w, o, what in zip(got, want, orc, ("word", "node", "weight")):
            assert np.array_equal(g, w) and np.array_equal(g, o), f"{name}, levelsup {levelsup}: {what}"
    for f, level, p, q in s.ties:                                    # spelled out: the planted ties went to the first sibling
        assert voc.descend(s.features[f:f + 1], 0)[0][0] == ref.descent_of(s, 0)[0][f]


@pytest.mark.parametrize("name", list(TREES))
def test_descent_resident_batch(name):
    """orbm_bow_transform_batch_dev: counts cap, 0, 1, 15, 16, 17 (one 16-lane row short, full, and one over), one count above cap
    and one negative (the kernel clamps both), rows past the count untouched."""
    import torch
    s = TREES[name]
    voc = vocabulary(name)
    n = len(s.features)
    cap = 150
    counts = [cap, 0, 1, 15, 16, 17, cap + 7, -3]
    used = [min(max(c, 0), cap) for c in counts]
    # set k = a window of the features ending at the planted ones (the last rows), shifted by k * 37
    index = np.stack([(n - cap - 37 * k + np.arange(cap)) % n for k in range(len(counts))])
    sets = np.ascontiguousarray(s.features[index])
    d = torch.from_numpy(sets).cuda(); c = torch.tensor(counts, dtype=torch.int32).cuda()
    for levelsup in (0, 1):
        w = torch.full((len(counts), cap), -9, dtype=torch.int32).cuda(); nd = torch.full_like(w, -9)
        voc.descend_batch_device(d.data_ptr(), c.data_ptr(), cap, len(counts), levelsup, w.data_ptr(), nd.data_ptr())
        torch.cuda.synchronize()
        w, nd = w.cpu().numpy(), nd.cpu().numpy()
        rw, rn, _, _ = ref.descent_of(s, levelsup)
        for k, cnt in enumerate(used):
            ow, on, _ = oracle.bow_descend(*s.tree, sets[k, :cnt], levelsup)
            assert np.array_equal(w[k, :cnt], rw[index[k, :cnt]]) and np.array_equal(nd[k, :cnt], rn[index[k, :cnt]]), f"set {k}"
            assert np.array_equal(w[k, :cnt], ow) and np.array_equal(nd[k, :cnt], on), f"set {k}"
            assert (w[k, cnt:] == -9).all() and (nd[k, cnt:] == -9).all(), f"set {k}: rows past the count"


@pytest.mark.parametrize("name", ["20x20x3", "irregular"])
def test_vocabulary_transform_every_scoring_and_weighting(name):
    """ORBVocabulary.transform (device descent + host assembly) against the reference's own descent and its second restatement of
    the BowVector, for the 6 scorings x 4 weightings."""
    s = TREES[name]
    word, node, _, _ = ref.descent_of(s, 1)
    for weighting in range(4):
        voc = vocabulary(name, weighting)
        w = voc.node_weight[np.nonzero(voc.node_word >= 0)[0]][word]
        for scoring in range(6):
            voc.m_scoring = scoring
            bow, fv = voc.transform(s.features, 1)
            rb, rf = ref.bow_vector(word, node, w, scoring, weighting)
            assert bow == rb and fv == rf and len(bow) > 100, (scoring, weighting)
        voc.m_scoring = 0


# ------------------------------------------------------------------------------------------------------------- distinctive
@functools.lru_cache(maxsize=None)
def distinctive_truth():
    desc, off, where = scenes.distinctive_batch()
    best = ref.distinctive(desc, off)
    assert np.array_equal(best, oracle.distinctive_descriptors(desc, off))
    best.setflags(write=False)
    return desc, off, where, best


def test_distinctive_whole_batch_in_one_call():
    desc, off, where, best = distinctive_truth()
    got = ORBmatcher.distinctive_descriptors(desc, off)
    names = [n for n, _, _ in scenes.distinctive_groups()]
    wrong = [names[where.index(i)] if i in where else f"empty point {i}" for i in np.nonzero(got != best)[0]]
    assert not wrong, wrong
    for (name, g, want), at in zip(scenes.distinctive_groups(), where):
        if want is not None:
            assert got[at] == want, name


def test_distinctive_does_not_depend_on_the_place_in_the_batch():
    answers = []
    for desc, off, pos in scenes.distinctive_placements():
        got = ORBmatcher.distinctive_descriptors(desc, off)
        assert np.array_equal(got, ref.distinctive(desc, off)) and np.array_equal(got, oracle.distinctive_descriptors(desc, off))
        answers.append(list(got[pos]))
    assert answers[0] == answers[1] == answers[2] and answers[0][0] == 64 and answers[0][2] == 128


def test_distinctive_one_point_and_the_observation_limit():
    desc, off, where, best = distinctive_truth()
    names = [n for n, _, _ in scenes.distinctive_groups()]
    for name in ("random 1", "random 128", "planted row 127 of 128", "planted row 128 of 129", "random 257"):
        at = where[names.index(name)]
        one = ORBmatcher.distinctive_descriptors(desc[off[at]:off[at + 1]], np.array([0, off[at + 1] - off[at]], np.int32))
        assert list(one) == [best[at]], name
    assert list(ORBmatcher.distinctive_descriptors(np.zeros((0, 32), np.uint8), np.array([0, 0], np.int32))) == [-1]
    # 65,536 observations of one point: refused before anything is staged or launched
    # (65,535 itself is inside the limit and is not run: one workgroup would walk N^2 / 64 wave iterations)
    L = lib()
    big = np.zeros((65539, 32), np.uint8); o = np.array([0, 3, 65539], np.int32); out = np.full(2, -7, np.int32)
    assert L.orbm_distinctive_descriptors(ptr(big), ptr(o), 2, ptr(out)) == ERR_UNSUPPORTED
    assert b"65,535" in L.orbx_last_error() and list(out) == [-7, -7]


# ------------------------------------------------------------------------------------------------------------- candidate lists
def test_candidate_lists_at_the_workgroup_edge():
    m = ORBmatcher()
    for k, (A, B, off, idx, planted) in enumerate(scenes.candidate_scenes()):
        got = m.match_candidates(A, B, off, idx)
        want = ref.match_candidates(A, B, off, idx)
        orc = oracle.match_candidates(A, B, off, idx)
        for g, w, o, what in zip(got, want, orc, ("best", "second", "idx")):
            assert np.array_equal(g, w) and np.array_equal(g, o), f"scene {k} (nA = {len(A)}): {what}"
        for i, kind in planted.items():
            if kind == "complement":
                assert (got[0][i], got[1][i]) == (256, INT_MAX)
            else:
                assert got[1][i] == got[0][i] and got[2][i] == idx[off[i]]


def test_candidate_lists_documented_refusals():
    A, B, off, idx, _ = scenes.candidate_scenes()[5]
    m = ORBmatcher()
    for bad in (len(B), -1, 2 ** 31 - 1):
        ix = idx.copy(); ix[len(ix) // 2] = bad
        with pytest.raises(OrbxError) as e:
            m.match_candidates(A, B, off, ix)
        assert e.value.code == ERR_ARG and "out of range" in str(e.value)
    o = off.copy(); k = int(np.nonzero(np.diff(off) == 40)[0][0]); o[k + 1] = o[k] - 1
    with pytest.raises(OrbxError) as e:
        m.match_candidates(A, B, o, idx)
    assert e.value.code == ERR_ARG and "monotone" in str(e.value)
    L = lib()                                                        # the outputs of a refused call are not touched
    out = [np.full(len(A), -7, np.int32) for _ in range(3)]
    ix = idx.copy(); ix[0] = len(B)
    assert L.orbm_match_candidates(ptr(A), len(A), ptr(B), len(B), ptr(off), ptr(ix), *[ptr(x) for x in out]) == ERR_ARG
    assert all((x == -7).all() for x in out)


# ------------------------------------------------------------------------------------------------------------- Hamming matrix
def test_hamming_matrix_shapes_and_extreme_distances():
    for A, B in scenes.hamming_scenes():
        got = ORBmatcher.hamming_matrix(A, B)
        assert got.dtype == np.uint16 and np.array_equal(got, ref.hamming(A, B)) and np.array_equal(got, oracle.hamming_matrix(A, B))
        assert (got == 256).any()


@pytest.mark.parametrize("rows_first", [True, False])
def test_hamming_matrix_more_rows_than_a_grid_has_in_y(rows_first):
    """70,000 x 1 (the rows were the grid's y dimension: the kernel strides over them now) and 1 x 70,000."""
    A, B = scenes.hamming_long(70000, 9)
    want = ref.hamming(A, B)
    assert want[65535, 0] == 256 and want[65536, 0] == 0 and want[69999, 0] == 0 and want[69998, 0] == 256
    got = ORBmatcher.hamming_matrix(A, B) if rows_first else ORBmatcher.hamming_matrix(B, A).T
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------- y-dimension limits
def test_match_batch_pair_limit():
    """orbm_match_batch_dev: 65,535 pairs run; 65,536 are refused with ORBX_ERR_UNSUPPORTED, nothing queued (not even the clearing
    of nmatch), and the message names the limit."""
    import torch
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (2, 1, 32), dtype=np.uint8)
    n = 65536
    d = torch.from_numpy(desc).cuda(); c = torch.ones(2, dtype=torch.int32).cuda()
    pa = torch.zeros(n, dtype=torch.int32).cuda(); pb = torch.ones(n, dtype=torch.int32).cuda()
    out = [torch.full((n, 1), -7, dtype=torch.int32).cuda() for _ in range(4)]
    nm = torch.full((n,), -7, dtype=torch.int32).cuda()
    m = ORBmatcher(0.6)
    args = lambda k: (d.data_ptr(), c.data_ptr(), 1, pa.data_ptr(), pb.data_ptr(), k, *[o.data_ptr() for o in out], nm.data_ptr())
    with pytest.raises(OrbxError) as e:
        m.match_batch_device(*args(n), th=256)
    torch.cuda.synchronize()
    assert e.value.code == ERR_UNSUPPORTED and "65,535" in str(e.value)
    assert all(bool((o == -7).all()) for o in out) and bool((nm == -7).all())
    m.match_batch_device(*args(n - 1), th=256)
    torch.cuda.synchronize()
    dist = int(ref.hamming(desc[0], desc[1])[0, 0])
    best, second, idx, m12 = (o.cpu().numpy()[:, 0] for o in out)
    assert (best[:n - 1] == dist).all() and (second[:n - 1] == INT_MAX).all() and (idx[:n - 1] == 0).all() and (m12[:n - 1] == 0).all()
    assert (nm.cpu().numpy()[:n - 1] == 1).all()
    assert best[n - 1] == -7 and int(nm[n - 1]) == -7


def test_bow_batch_set_limit():
    """orbm_bow_transform_batch_dev: 65,535 sets run; 65,536 are refused the same way."""
    import torch
    s = TREES["16x17"]
    voc = vocabulary("16x17")
    n = 65536
    pick = np.arange(n) % len(s.features)
    d = torch.from_numpy(np.ascontiguousarray(s.features[pick][:, None, :])).cuda()
    c = torch.ones(n, dtype=torch.int32).cuda()
    w = torch.full((n, 1), -9, dtype=torch.int32).cuda(); nd = torch.full_like(w, -9)
    with pytest.raises(OrbxError) as e:
        voc.descend_batch_device(d.data_ptr(), c.data_ptr(), 1, n, 0, w.data_ptr(), nd.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == ERR_UNSUPPORTED and "65,535" in str(e.value)
    assert bool((w == -9).all()) and bool((nd == -9).all())
    voc.descend_batch_device(d.data_ptr(), c.data_ptr(), 1, n - 1, 0, w.data_ptr(), nd.data_ptr())
    torch.cuda.synchronize()
    rw, rn, _, _ = ref.descent_of(s, 0)
    w, nd = w.cpu().numpy()[:, 0], nd.cpu().numpy()[:, 0]
    assert np.array_equal(w[:n - 1], rw[pick[:n - 1]]) and np.array_equal(nd[:n - 1], rn[pick[:n - 1]])
    assert w[n - 1] == -9 and nd[n - 1] == -9
