"""Plain numpy restatement of the four descriptor-set operations, written from the reference's sources (paths relative to
the ORB_SLAM2_E tree) and from nothing else:

* hamming            -- ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1848-1864): the number of differing bits.
* distinctive        -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:305-370).
* match_candidates   -- the best / second-best update every Search* shares (e.g. src/ORBmatcher.cc:664-672).
* bow_descend        -- TemplatedVocabulary::transform for one feature (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1262).
* bow_vector         -- TemplatedVocabulary::transform for a frame (:1127-1195) with BowVector::addWeight / addIfNotExist /
                        normalize (BowVector.cpp:34-84), the std::map kept as a sorted key list.

Everything is integer arithmetic or a double sum in the reference's order, so the comparisons made with it are exact."""
import bisect
import math

import numpy as np

INT_MAX = 2 ** 31 - 1

# DBoW2 enumerators (BowVector.h:36-53)
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5


def hamming(A, B):
    """[nA][nB] int32: bits set in A[i] xor B[j].  Rows of A are taken a few at a time to bound the unpacked size."""
    A = np.asarray(A, np.uint8).reshape(-1, 32); B = np.asarray(B, np.uint8).reshape(-1, 32)
    out = np.zeros((len(A), len(B)), np.int32)
    if len(A) == 0 or len(B) == 0:
        return out
    step = max(1, (1 << 19) // len(B))
    for r in range(0, len(A), step):
        x = A[r:r + step, None, :] ^ B[None, :, :]
        out[r:r + step] = np.unpackbits(x, axis=2).sum(axis=2, dtype=np.int32)
    return out


def distinctive_medians(d, dist=hamming):
    """The sorted-row medians of one map point's observations (MapPoint.cc:338-357): Distances[i][i] = 0, the row sorted,
    element int(0.5 * (N - 1))."""
    N = len(d)
    D = dist(d, d)
    np.fill_diagonal(D, 0)
    return np.sort(D, axis=1)[:, int(0.5 * (N - 1))]


def distinctive(desc, off):
    """best[i] = the row (within point i) whose median distance to the point's rows is least; `median < BestMedian`, so
    the first row wins a tie (:359-363); -1 for a point without observations (the reference returns early, :332)."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    best = np.full(len(off) - 1, -1, np.int32)
    for i in range(len(off) - 1):
        d = desc[off[i]:off[i + 1]]
        if len(d) == 0:
            continue
        BestMedian, BestIdx = INT_MAX, 0
        for a, median in enumerate(distinctive_medians(d)):
            if median < BestMedian:
                BestMedian, BestIdx = int(median), a
        best[i] = BestIdx
    return best


def match_candidates(A, B, off, idx):
    """Per query i over its candidates idx[off[i]:off[i + 1]] in list order:
    if(dist<bestDist){bestDist2=bestDist;bestDist=dist;bestIdx=j;} else if(dist<bestDist2) bestDist2=dist;"""
    A = np.asarray(A, np.uint8).reshape(-1, 32); B = np.asarray(B, np.uint8).reshape(-1, 32)
    nA = len(A)
    best = np.zeros(nA, np.int32); second = np.zeros(nA, np.int32); arg = np.zeros(nA, np.int32)
    for i in range(nA):
        bestDist, bestDist2, bestIdx = INT_MAX, INT_MAX, -1
        for k in range(off[i], off[i + 1]):
            j = int(idx[k])
            dist = int(np.unpackbits(A[i] ^ B[j]).sum())
            if dist < bestDist:
                bestDist2 = bestDist; bestDist = dist; bestIdx = j
            elif dist < bestDist2:
                bestDist2 = dist
        best[i], second[i], arg[i] = bestDist, bestDist2, bestIdx
    return best, second, arg


def bow_descend(tree, features, levelsup, trace=None):
    """tree = (child_off, child_ids, node_desc, node_word, node_weight, L), the flat arrays orbm_vocab_create takes.
    Returns (word id, node id at level L - levelsup, word weight) per feature.  `trace`, if a list, receives per feature
    the child positions taken, one per level (for the scenes' own conditions; not part of the operation)."""
    child_off, child_ids, node_desc, node_word, node_weight, L = tree
    features = np.asarray(features, np.uint8).reshape(-1, 32)
    n = len(features)
    word = np.zeros(n, np.int32); node = np.zeros(n, np.int32); weight = np.zeros(n, np.float64)
    nid_level = L - levelsup
    for f in range(n):
        nid = 0                                   # `if(nid_level <= 0) *nid = 0` (:1227); 0 also where a leaf comes before that level (:1151 leaves it unset)
        final_id, current_level = 0, 0
        path = []
        while True:
            current_level += 1
            nodes = child_ids[child_off[final_id]:child_off[final_id + 1]]
            d = np.unpackbits(features[f][None, :] ^ node_desc[nodes], axis=1).sum(axis=1)
            final_id = int(nodes[0]); best_d = int(d[0]); pos = 0
            for p in range(1, len(nodes)):
                if d[p] < best_d:
                    best_d = int(d[p]); final_id = int(nodes[p]); pos = p
            path.append(pos)
            if current_level == nid_level:
                nid = final_id
            if child_off[final_id + 1] == child_off[final_id]:     # isLeaf(): no children
                break
        word[f], node[f], weight[f] = node_word[final_id], nid, node_weight[final_id]
        if trace is not None:
            trace.append(path)
    return word, node, weight


_DESCENTS = {}


def descent_of(scene, levelsup):
    """(word, node, weight, trace) of a tree scene (descriptor_sets_scenes.TreeScene): computed once per process, read-only."""
    key = (scene.name, levelsup)
    if key not in _DESCENTS:
        trace = []
        out = bow_descend(scene.tree, scene.features, levelsup, trace)
        for a in out:
            a.setflags(write=False)
        _DESCENTS[key] = out + (trace,)
    return _DESCENTS[key]


class _Map:
    """std::map<unsigned, T> as a sorted key list and a value list: lower_bound is bisect_left."""

    def __init__(self):
        self.keys, self.vals = [], []

    def lower_bound(self, k):
        return bisect.bisect_left(self.keys, k)

    def found(self, it, k):
        return it < len(self.keys) and self.keys[it] == k

    def insert(self, it, k, v):
        self.keys.insert(it, k); self.vals.insert(it, v)


def bow_vector(word, node, w, scoring=L1_NORM, weighting=TF_IDF):
    """(BowVector as {word id: value}, FeatureVector as {node id: [feature indices]}) of one frame."""
    v, fv = _Map(), _Map()
    add_weight = weighting in (TF, TF_IDF)
    must = scoring != DOT_PRODUCT                 # ScoringObject.h:74-89: every scoring but DOT_PRODUCT normalises
    l2 = scoring == L2_NORM                       # ... and only L2_NORM with the L2 norm
    for i_feature in range(len(word)):
        if not w[i_feature] > 0:                  # stopped
            continue
        wid = int(word[i_feature])
        it = v.lower_bound(wid)
        if v.found(it, wid):
            if add_weight:
                v.vals[it] += float(w[i_feature])                  # addWeight; addIfNotExist leaves the first value
        else:
            v.insert(it, wid, float(w[i_feature]))
        nid = int(node[i_feature])
        it = fv.lower_bound(nid)
        if fv.found(it, nid):
            fv.vals[it].append(i_feature)
        else:
            fv.insert(it, nid, [i_feature])
    if add_weight and v.keys and not must:
        nd = float(len(v.keys))
        v.vals = [x / nd for x in v.vals]
    if must:
        norm = 0.0
        for x in v.vals:                          # begin() .. end(): ascending word id
            norm += x * x if l2 else math.fabs(x)
        if l2:
            norm = math.sqrt(norm)
        if norm > 0.0:
            v.vals = [x / norm for x in v.vals]
    return dict(zip(v.keys, v.vals)), dict(zip(fv.keys, fv.vals))


def bow_vector_fsum(word, w, scoring=L1_NORM, weighting=TF_IDF):
    """The BowVector's values once more with every sum correctly rounded (math.fsum): the yardstick for the one derived bound,
    n * 2^-52 relative, of a sequential sum of n positive doubles."""
    add_weight = weighting in (TF, TF_IDF)
    terms = {}
    for i in range(len(word)):
        if w[i] > 0:
            terms.setdefault(int(word[i]), []).append(float(w[i]))
    vals = {k: (math.fsum(t) if add_weight else t[0]) for k, t in terms.items()}
    if scoring == DOT_PRODUCT:
        if add_weight and vals:
            vals = {k: x / len(vals) for k, x in vals.items()}
        return vals
    if scoring == L2_NORM:
        norm = math.sqrt(math.fsum(x * x for x in vals.values()))
    else:
        norm = math.fsum(abs(x) for x in vals.values())
    return {k: x / norm for k, x in vals.items()} if norm > 0.0 else vals
