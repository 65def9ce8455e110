"""Scenes for the batched SearchByBoW (orbm_frame_search_by_bow_pairs): a Side is one frame's share of a search (keypoints,
descriptors, FeatureVector, "owns a good MapPoint" mask), a Pair two Sides.  A Side that stands in several Pairs is ONE resident
frame on the device.  Everything here is checked on oracle.search_by_bow alone by tests/test_cpu_bow_pairs.py; the GPU tests
(tests/test_gpu_bow_pairs.py) compare the library with it."""
import numpy as np

import oracle
import selection_scenes as S
from orb_slam2_e_amd.synth import synth_bow_case
from orb_slam2_e_amd.vocabulary import feature_vector_arrays

BOUNDS = S.BOUNDS
TH_LOW = 45
RES_T, RES_QREG, RES_MAXIT = 1024, 2, 48         # k_resolve_par's: threads, queries a thread keeps in registers, iteration limit
MANY = (7, 2654)                                # synth_bow_case(seed, n1): RES_T * RES_QREG + 1 valid queries in the Frame form


class Side:
    def __init__(self, desc, angle, fv, valid, kps=None):
        self.desc = np.ascontiguousarray(desc, np.uint8)
        self.angle = np.ascontiguousarray(angle, np.float32)
        self.fv = tuple(np.ascontiguousarray(a, np.int32) for a in fv)
        self.valid = np.ascontiguousarray(valid, np.uint8)
        self.n = len(self.desc)
        if kps is None:                          # positions are not read by SearchByBoW: a row of keypoints inside the grid
            kps = np.zeros(self.n, oracle.KP_DTYPE)
            kps["x"] = 20.0 + 0.05 * np.arange(self.n); kps["y"] = 100.0; kps["size"] = 31.0
            kps["angle"] = self.angle
        self.kps = kps
        self._frame = None

    def frame(self):
        """the resident frame, made on first use (GPU tests only) and kept until close_frames"""
        if self._frame is None:
            from orb_slam2_e_amd import Frame
            self._frame = Frame(self.kps, self.desc, BOUNDS)
            _OPEN.append(self)
        return self._frame


_OPEN = []


def close_frames():
    for s in _OPEN:
        s._frame.close(); s._frame = None
    del _OPEN[:]


class Pair:
    def __init__(self, s1, s2, name=""):
        self.s1, self.s2, self.name = s1, s2, name
        self._ref = {}

    def args(self):
        """the pair as ORBmatcher.frame_search_by_bow_pairs / frame_search_by_bow take it"""
        return (self.s1.frame(), self.s1.fv, self.s1.valid, self.s2.frame(), self.s2.fv, self.s2.valid)

    def oracle(self, kf_kf, ratio, ori):
        """(match12, match21, nmatches) of the reference's loop, computed once per setting"""
        key = (bool(kf_kf), float(ratio), bool(ori))
        if key not in self._ref:
            a, b = self.s1, self.s2
            self._ref[key] = oracle.search_by_bow(a.fv, a.valid, a.desc, a.angle, b.fv, b.valid if kf_kf else None, b.desc, b.angle,
                                                  kf_kf, ratio, ori)
        return self._ref[key]

    def nqueries(self):
        """queries of the search in the Frame form: the valid features of the first set in nodes both sets hold"""
        n1, o1, i1 = self.s1.fv
        return int(sum(self.s1.valid[i1[o1[a]:o1[a + 1]]].sum() for a in np.nonzero(np.isin(n1, self.s2.fv[0]))[0]))


def sides_of_case(case):
    d1, a1, node1, keep1, valid1, d2, a2, node2, keep2, valid2 = case
    return Side(d1, a1, feature_vector_arrays(node1, keep1), valid1), Side(d2, a2, feature_vector_arrays(node2, keep2), valid2)


def case_pair(seed, n1=300, n2=320, nnodes=12, name=None):
    return Pair(*sides_of_case(synth_bow_case(seed, n1, n2, nnodes)), name=name or f"case{seed}_{n1}x{n2}")


def _noisy(desc, seed, on=True):
    """every descriptor with each bit flipped with probability 1 %"""
    if not on:
        return desc
    rng = np.random.default_rng(1000 + seed)
    return desc ^ np.packbits(rng.random((len(desc), 256)) < 0.01, axis=1, bitorder="little")


def shared_second(seeds, n1=300, n2=320, nnodes=12, noise=True):
    """Relocalisation's shape: ONE second frame (the current frame) in every pair.  The shared frame and the nodes are those of the
    first seed's case; pair k's first frame is that case's first set under seed k's bit noise, with seed k's valid and stop-word
    masks (unrelated descriptors of another seed would leave nothing to match).  noise = False: the masks alone differ."""
    base = synth_bow_case(seeds[0], n1, n2, nnodes)
    _, cur = sides_of_case(base)
    out = []
    for k in seeds:
        c = synth_bow_case(k, n1, n2, nnodes)
        out.append(Pair(Side(_noisy(base[0], k, noise), base[1], feature_vector_arrays(base[2], c[3]), c[4]), cur, f"shared_second_{k}"))
    return out


def shared_first(seeds, n1=300, n2=320, nnodes=12):
    """Loop closing's shape: ONE first frame (the current keyframe) in every pair; pair k's second frame is the first seed's second
    set under seed k's bit noise with seed k's masks."""
    base = synth_bow_case(seeds[0], n1, n2, nnodes)
    cur, _ = sides_of_case(base)
    out = []
    for k in seeds:
        c = synth_bow_case(k, n1, n2, nnodes)
        out.append(Pair(cur, Side(_noisy(base[5], k), base[6], feature_vector_arrays(base[7], c[8]), c[9]), f"shared_first_{k}"))
    return out


def turned(pair, degrees):
    """the pair with its second frame's angles shifted: another dominant bin of the rotation histogram"""
    b = pair.s2
    return Pair(pair.s1, Side(b.desc, (b.angle + np.float32(degrees)) % np.float32(360), b.fv, b.valid), pair.name + f"_turned{degrees}")


def selection_pair(kf_kf=False, ratio=0.6):
    """selection_scenes.scene("bow") for the form (its threshold islands sit at the form's threshold): list lengths 1 .. 300 either
    side of wave_topk's 256, claims at queries 62 - 65 of a node.  Returns the pair and its expected rows."""
    sc = S.scene("bow", S.RATIO, S.TH_LOW - 1 if kf_kf else S.TH_LOW, ratio)
    fv1, fv2 = sc.bow()
    k1, _ = sc.init_queries()
    return Pair(Side(sc.qdesc, sc.qangle, fv1, np.ones(sc.nq, np.uint8), k1),
                Side(sc.desc, sc.kps["angle"], fv2, np.ones(len(sc.kps), np.uint8), sc.kps), "selection"), sc.expect_bow(kf_kf, ratio)


def special_pair(kf_kf):
    """selection_scenes.bow_special and its expected rows"""
    a, want = S.bow_special(kf_kf)
    z = lambda d: np.zeros(len(d), np.float32)
    return Pair(Side(a["desc1"], z(a["desc1"]), a["fv1"], a["valid1"]), Side(a["desc2"], z(a["desc2"]), a["fv2"], a["valid2"]), "special"), want


def disjoint_pair(seed=5):
    """no node in common: no query"""
    p = case_pair(seed, 60, 70, 4)
    nodes, off, items = p.s2.fv
    return Pair(p.s1, Side(p.s2.desc, p.s2.angle, (nodes + 1, off, items), p.s2.valid), "disjoint")


def empty_pair(seed=6):
    """an empty first frame"""
    p = case_pair(seed, 60, 70, 4)
    e = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    return Pair(Side(np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), e, np.zeros(0, np.uint8)), p.s2, "empty")


def many_pair():
    """RES_T * RES_QREG + 1 = 2049 valid queries: the last one lives in global memory"""
    seed, n1 = MANY
    p = case_pair(seed, n1, n1 + 100, 90, "many")
    assert p.nqueries() == RES_T * RES_QREG + 1, p.nqueries()
    return p


def _flip(bits, idx):
    out = bits.copy()
    out[idx] ^= 1
    return out


def chain_pair(nchain, seed=11, ratio=0.75):
    """A dependency chain under the RATIO rule, nchain queries in ONE node: a seeded bit walk s_0, s_1, ... (40 bits flipped per
    step) is the second set; query 0 is at distance 10 of s_0, query i at distance 10 of s_{i-1} and 30 of s_i.  Sequentially query
    i finds s_{i-1} taken and accepts s_i (30 < ratio * the next free distance); the fixed point starts with every query on
    s_{i-1} and settles one query per iteration.  Asserts the distances, that every other member is far enough for both ratio
    tests (best 10 and best 30) and that the oracle gives match12[i] = i."""
    rng = np.random.default_rng(seed)
    s = [rng.integers(0, 2, 256).astype(np.uint8)]
    q = [_flip(s[0], rng.choice(256, 10, replace=False))]
    for i in range(1, nchain):
        step = rng.choice(256, 40, replace=False)
        s.append(_flip(s[i - 1], step))
        q.append(_flip(s[i - 1], step[:10]))
    pk = lambda rows: np.stack([np.packbits(r, bitorder="little") for r in rows])
    d1, d2 = pk(q), pk(s)
    dist = np.array([[S.hamming(a, b) for b in d2] for a in d1])
    for i in range(nchain):
        others = np.delete(dist[i], [i - 1, i] if i else [0])
        assert dist[i, i] == (30 if i else 10) and (i == 0 or dist[i, i - 1] == 10)
        assert others.size == 0 or others.min() * ratio > 30, (i, others.min())
    assert 10 < ratio * 30 and 30 <= TH_LOW - 1
    node = np.array([17], np.int32)
    fv = lambda n: (node, np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
    ones = lambda n: np.ones(n, np.uint8)
    p = Pair(Side(d1, np.zeros(nchain, np.float32), fv(nchain), ones(nchain)), Side(d2, np.zeros(nchain, np.float32), fv(nchain), ones(nchain)),
             f"chain{nchain}")
    for kf_kf in (False, True):
        m12, m21, nm = p.oracle(kf_kf, ratio, False)
        assert nm == nchain and np.array_equal(m12, np.arange(nchain)) and np.array_equal(m21, np.arange(nchain))
    return p
