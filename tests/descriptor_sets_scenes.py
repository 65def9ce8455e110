"""Seeded inputs for the descriptor-set kernels (k_bow_transform, k_distinctive, k_match_cands, k_hamming_matrix) at their tiling
edges.  Everything is small and generated; nothing is read from a file.  What each scene is FOR is asserted, on the numpy
reference alone, in tests/test_cpu_descriptor_sets.py."""
import functools

import numpy as np

INT_MAX = 2 ** 31 - 1


def _noise(rng, shape, p):
    """Random 256-bit rows (as [..., 32] bytes) with every bit set with probability p."""
    return np.packbits(rng.random(tuple(shape) + (256,)) < p, axis=-1, bitorder="little")


def _flip_bits(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _diff_bits(a, b):
    return np.nonzero(np.unpackbits(a ^ b, bitorder="little"))[0]


# ------------------------------------------------------------------------------------------------------------- vocabulary trees
class Tree:
    """A vocabulary tree under construction: nodes in breadth-first creation order, children of a node consecutive."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parent, self.depth, self.desc, self.kids = [0], [0], [self.rng.integers(0, 256, 32, dtype=np.uint8)], [[]]

    def add_children(self, p, k):
        d = self.depth[p] + 1
        for _ in range(k):
            self.parent.append(p); self.depth.append(d); self.kids.append([])
            self.desc.append(self.desc[p] ^ _noise(self.rng, (), 0.5 ** d))
            self.kids[p].append(len(self.parent) - 1)
        return self.kids[p]

    def equal_siblings(self, node, p, q):
        """Child q of `node` gets child p's descriptor: strict '<' must keep p."""
        self.desc[self.kids[node][q]] = self.desc[self.kids[node][p]].copy()

    def even_apart(self, node, p, q):
        """Make children p and q of `node` differ in an even number of bits, so that a feature can sit at the same distance from both."""
        a, b = self.kids[node][p], self.kids[node][q]
        if len(_diff_bits(self.desc[a], self.desc[b])) % 2:
            same = np.nonzero(np.unpackbits(self.desc[a] ^ self.desc[b], bitorder="little") == 0)[0]
            self.desc[b] = _flip_bits(self.desc[b], [int(same[0])])

    def complement_children(self, node):
        """Every child of `node` becomes the complement of `node`'s own descriptor: the node's descriptor, as a feature, arrives at
        the node and is 256 bits from each child."""
        for c in self.kids[node]:
            self.desc[c] = ~self.desc[node]

    def arrays(self, L, seed):
        n = len(self.parent)
        rng = np.random.default_rng(seed)
        off, ids = [0], []
        for i in range(n):
            ids += self.kids[i]; off.append(len(ids))
        leaf = np.array([not k for k in self.kids])
        word = np.full(n, -1, np.int32); word[leaf] = np.arange(int(leaf.sum()))
        weight = np.where(leaf, rng.uniform(0.25, 8.0, n), 0.0)
        weight[np.nonzero(leaf)[0][5::11]] = 0.0                     # stop words
        return (np.array(off, np.int32), np.array(ids, np.int32), np.stack(self.desc), word, weight, L)


def _tie_feature(desc, kids, p, q):
    """A feature at the same distance from children p and q (which differ in an even number of bits): child p with half of
    the differing bits flipped."""
    diff = _diff_bits(desc[kids[p]], desc[kids[q]])
    assert len(diff) % 2 == 0 and len(diff) > 0
    return _flip_bits(desc[kids[p]], [int(b) for b in diff[:len(diff) // 2]])


class TreeScene:
    """tree: the flat arrays; features [n][32]; ties: [(feature index, level (1-based), position that must win, position it ties
    with)]; all256: [(feature index, level)] -- features that are 256 bits from every child at that level; L; name."""

    def __init__(self, name, tree, features, ties, all256):
        self.name, self.tree, self.features, self.ties, self.all256 = name, tree, features, ties, all256
        self.L = tree[5]
        self.levelsups = sorted({0, 1, self.L - 1, self.L, self.L + 1})

    def with_weighting(self, weighting):
        """The same tree with the word weights a vocabulary of that WeightingType holds: 1 for TF and BINARY (a stopped word keeps 0)."""
        off, ids, desc, word, weight, L = self.tree
        if weighting in (1, 3):
            weight = np.where(weight > 0, 1.0, 0.0)
        return (off, ids, desc, word, weight, L)


def _finish(name, t, L, seed, root_ties, equal, complement_nodes):
    """equal: [(node, p, q)] planted equal siblings; root_ties: [(p, q)] pairs of root children a feature sits between;
    complement_nodes: nodes whose children all become the complement of the node."""
    for p, q in root_ties:
        t.even_apart(0, p, q)
    for node, p, q in equal:
        t.equal_siblings(node, p, q)
    for node in complement_nodes:
        t.complement_children(node)
    tree = t.arrays(L, seed + 1)
    off, ids, desc, word, weight, _ = tree
    rng = np.random.default_rng(seed + 2)
    leaves = np.nonzero(word >= 0)[0]
    own = desc[leaves]
    feats = [own, own ^ _noise(rng, (len(leaves),), 0.04)]            # every leaf's descriptor, and one noisy copy of each
    extra, ties, all256 = [], [], []
    base = 2 * len(leaves)
    for p, q in root_ties:
        ties.append((base + len(extra), 1, p, q)); extra.append(_tie_feature(desc, t.kids[0], p, q))
    for node, p, q in equal:                                          # the shared descriptor itself, aimed at that node
        ties.append((base + len(extra), t.depth[node] + 1, p, q)); extra.append(desc[t.kids[node][q]])
    for node in complement_nodes:
        all256.append((base + len(extra), t.depth[node] + 1)); extra.append(desc[node])
    feats.append(np.stack(extra))
    return TreeScene(name, tree, np.ascontiguousarray(np.concatenate(feats)), ties, all256)


def _uniform(name, widths, seed, root_ties, plant):
    """A tree with widths[d] children at every node of depth d.  plant(t, levels) -> (equal, complement_nodes), levels[d] = the
    nodes of depth d."""
    t = Tree(seed)
    levels = [[0]]
    for k in widths:
        levels.append([c for p in levels[-1] for c in t.add_children(p, k)])
    equal, comp = plant(t, levels)
    return _finish(name, t, len(widths), seed, root_ties, equal, comp)


def _irregular(seed=40):
    """Nodes of 1, 15, 16, 17, 31, 32, 33 and 48 children; leaves at depths 1, 2 and 3, interleaved in the feature order so that
    the four features of one wave leave the descent loop at different levels."""
    t = Tree(seed)
    top = t.add_children(0, 17)
    second = {}
    for c, k in zip(top[:8], (1, 15, 16, 31, 32, 33, 48, 17)):       # the other nine root children are leaves at depth 1
        second[k] = t.add_children(c, k)
    for k, kids in second.items():                                    # first and last child of each carry a third level
        t.add_children(kids[0], 2)
        if k > 1:
            t.add_children(kids[-1], 17)
    n48, n33, n32, n31, n15 = top[6], top[5], top[4], top[3], top[1]
    equal = [(n48, 7, 23), (n48, 9, 41), (n48, 2, 17), (n48, 15, 16), (n33, 0, 32), (n33, 15, 16), (n32, 15, 31), (n31, 14, 30)]
    comp = [second[16][0]]                                            # a node of 2 children, at depth 2
    s = _finish("irregular", t, 3, seed, [(0, 16), (2, 9)], equal, comp)
    # interleave the depths: shuffled, neighbouring features end at different levels
    order = np.random.default_rng(seed + 3).permutation(len(s.features))
    inv = np.empty_like(order); inv[order] = np.arange(len(order))
    s.features = np.ascontiguousarray(s.features[order])
    s.ties = [(int(inv[f]), lv, p, q) for f, lv, p, q in s.ties]
    s.all256 = [(int(inv[f]), lv) for f, lv in s.all256]
    return s


@functools.lru_cache(maxsize=None)
def tree_scenes():
    """The wide trees of widths (16, 17), (17, 20), (33, 2), (20, 20, 3) and the irregular one.

    Equal siblings are planted only in nodes that are not alone on their level (in a level's only node an equal sibling would
    make its position unreachable for every feature): there the tie is made by a feature at the same distance from two
    different children.  The all-256 feature needs a one-chunk node below the root, which (33, 2), (20, 20, 3) and the
    irregular tree have."""
    def p_16_17(t, lv):
        a, b = lv[1][3], lv[1][9]
        return [(a, 0, 16), (b, 15, 16)], []

    def p_17_20(t, lv):
        a, b, c = lv[1][0], lv[1][8], lv[1][16]
        return [(a, 3, 19), (b, 2, 17), (c, 15, 16)], []

    def p_33_2(t, lv):
        return [], [lv[1][20]]

    def p_20_20_3(t, lv):
        a, b, c = lv[1][1], lv[1][10], lv[1][19]
        return [(a, 3, 19), (b, 2, 17), (c, 15, 16)], [lv[2][57]]

    return (
        _uniform("16x17", (16, 17), 10, [(2, 9)], p_16_17),
        _uniform("17x20", (17, 20), 20, [(0, 16), (2, 9)], p_17_20),
        _uniform("33x2", (33, 2), 30, [(5, 21), (0, 32), (2, 17), (15, 16), (16, 31)], p_33_2),
        _uniform("20x20x3", (20, 20, 3), 50, [(3, 19), (2, 17), (15, 16)], p_20_20_3),
        _irregular(),
    )


# ------------------------------------------------------------------------------------------------- observation groups (distinctive)
DD_SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 257, 700, 2000)
# bit-flip probabilities of the groups above 128 rows (the row-by-row path), spread so that the winning medians differ
_DD_LONG_P = {129: 0.06, 130: 0.11, 191: 0.16, 192: 0.08, 193: 0.13, 257: 0.19, 700: 0.10, 2000: 0.145}


def _group(rng, n, p, winner=None):
    """n rows = one base descriptor xor noise(p); `winner`: that row is the base itself."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    g = base[None, :] ^ _noise(rng, (n,), p)
    if winner is not None:
        g[winner] = base
    return g


@functools.lru_cache(maxsize=None)
def distinctive_groups():
    """[(name, rows [N][32], expected winner or None)].  None = whatever the reference says."""
    rng = np.random.default_rng(77)
    out = []
    for n in DD_SIZES:
        out.append((f"random {n}", _group(rng, n, _DD_LONG_P.get(n, 0.1)) if n else np.zeros((0, 32), np.uint8), -1 if n == 0 else None))
    for n, w in ((128, 63), (128, 64), (128, 127), (129, 128), (700, 699)):
        out.append((f"planted row {w} of {n}", _group(rng, n, 0.12 if n < 700 else 0.17, w), w))
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    out.append(("a and three complements", np.stack([a, ~a, ~a, ~a]), 1))
    out.append(("200 identical rows", np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 200, axis=0), 0))
    g = _group(rng, 100, 0.12, 70); g[5] = g[70]
    out.append(("two equal winners, short path", g, 5))
    g = _group(rng, 150, 0.12, 140); g[20] = g[140]
    out.append(("two equal winners, long path", g, 20))
    return tuple(out)


def concat_groups(groups, empties_between=True):
    """(desc [total][32], off [m + 1], index of each group's point in the batch)."""
    rows, sizes, where = [], [], []
    for g in groups:
        where.append(len(sizes)); sizes.append(len(g)); rows.append(g)
        if empties_between:
            sizes.append(0)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(rows)), off, where


def distinctive_batch():
    """Every group in one call, an empty point after each."""
    return concat_groups([g for _, g, _ in distinctive_groups()])


def distinctive_placements():
    """Three groups (short path, its upper half, long path) standing first, in the middle and last among filler points: the
    answer for a point must not depend on where it stands.  Returns [(desc, off, positions of the three)]."""
    named = {n: g for n, g, _ in distinctive_groups()}
    three = [named["planted row 64 of 128"], named["random 65"], named["planted row 128 of 129"]]
    rng = np.random.default_rng(78)
    filler = [_group(rng, int(n), 0.1) for n in rng.integers(1, 40, 9)]
    out = []
    for place in ("first", "middle", "last"):
        seq = {"first": three + filler, "middle": filler[:4] + three + filler[4:], "last": filler + three}[place]
        desc, off, where = concat_groups(seq, empties_between=False)
        start = {"first": 0, "middle": 4, "last": len(filler)}[place]
        out.append((desc, off, where[start:start + 3]))
    return out


# ------------------------------------------------------------------------------------------------------------- candidate lists
CAND_LENGTHS = (0, 1, 2, 40)


def candidate_scene(nA, rot, seed=0):
    """nA queries against 300 train rows; the list of query i has CAND_LENGTHS[(i + rot) % 4] entries.  The last queries (as many as
    nA allows) carry the planted lists: a candidate listed twice, two different candidates with equal descriptors, and one
    whose only candidate is the query's complement.  Returns (A, B, off, idx, planted) with planted = {query: kind}."""
    rng = np.random.default_rng(1000 * nA + 10 * rot + seed)
    nB = 300
    B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    A = B[rng.integers(0, nB - 10, nA)] ^ _noise(rng, (nA,), 0.08)
    lists = [rng.integers(0, nB - 10, CAND_LENGTHS[(i + rot) % 4]).tolist() for i in range(nA)]
    planted = {}
    kinds = ("twice", "equal pair", "complement")
    for k, kind in enumerate(kinds[rot % 3:] + kinds[:rot % 3]):
        i = nA - 1 - k
        if i < 0:
            break
        planted[i] = kind
        if kind == "twice":
            lists[i] = [17, 17]
        elif kind == "equal pair":
            B[nB - 1] = B[nB - 2]                 # rows 290.. are in no random list
            lists[i] = [nB - 1, nB - 2]
        else:
            B[nB - 3] = ~A[i]
            lists[i] = [nB - 3]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    idx = np.array([j for x in lists for j in x], np.int32)
    return A, B, off, idx, planted


@functools.lru_cache(maxsize=None)
def candidate_scenes():
    out = [candidate_scene(nA, rot) for nA in (1, 255, 256, 257) for rot in range(4)]
    rng = np.random.default_rng(5)                                    # nB = 0, every list empty
    out.append((rng.integers(0, 256, (5, 32), dtype=np.uint8), np.zeros((0, 32), np.uint8), np.zeros(6, np.int32), np.zeros(0, np.int32), {}))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------- Hamming matrix
HAMMING_SHAPES = ((1, 1), (1, 257), (3, 256), (300, 255))


@functools.lru_cache(maxsize=None)
def hamming_scenes():
    out = []
    for nA, nB in HAMMING_SHAPES:
        rng = np.random.default_rng(100 * nA + nB)
        A = rng.integers(0, 256, (nA, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
        if nB == 1:
            A[0] = ~B[0]                           # the only entry: 256
        else:
            B[0] = A[0]; B[nB - 1] = ~A[0]         # row 0 holds 0 and 256, at both ends
            if nA > 1:
                B[nB // 2] = ~A[nA - 1]; A[nA // 2] = B[nB - 2]          # ... and in the last and a middle row
        out.append((A, B))
    return tuple(out)


def hamming_long(n, seed):
    """n rows against one, for the row counts beyond a grid's y dimension: (A [n][32], B [1][32]), with 0 and 256 in the last rows."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (n, 32), dtype=np.uint8); B = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    A[n - 1] = B[0]; A[n - 2] = ~B[0]; A[65535] = ~B[0]; A[65536] = B[0]
    return A, B
