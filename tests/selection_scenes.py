"""Constructed cases for the selection core of the matcher (orbm_search.hip: wave_topk / wave_topk_regs, select_two,
accepts_projection / accepts_initialization, the claim table of k_resolve, the fixed points k_resolve_par / k_resolve_init_par,
and k_win_best's best / second), each with its expected result written down from the reference's rule
(src/ORBmatcher.cc:69-130, :384-456, :626-696, :745-828), not computed by the code under test.

How a case is made
  * Descriptors: a candidate is BASE with a chosen set S of bits flipped, a query is BASE with a set T flipped, so their
    Hamming distance is |S ^ T| exactly (a plain query has T = {}: distance |S|; all 256 bits = the complement: 256 - |S|).
    A "blocker" is a query with T = S of one candidate: distance 0 to it, so every rule accepts it there and the slot is
    taken for the queries behind it.
  * Order: an island's candidates sit in one grid column (or a run of columns: `split`), 64 to a cell, cell after cell down the
    column, keypoint indices ascending -- the visiting order of Frame::GetFeaturesInArea (column, row, index) is the order
    they were added in.  Every query of an island has the window that covers the island and nothing else.  In the BoW entries
    an island is one vocabulary node: its candidates are the node's members of the second set in that order.
  * Expectation: every query DECLARES which candidate is its best and which its second in the reference's loop, given what the
    queries before it took (`best`, `second`; `free` = the same when nothing blocks: qtakes = 0 and the uncoupled window /
    fuse searches).  The declared pair goes through the reference's acceptance rule restated in numpy float32 (accepts());
    `want` pins the decision where the case is about it.  tests/test_cpu_selection.py holds all of it against the C oracle's
    literal loops before anything runs on a GPU.
"""
import functools
import zlib
from fractions import Fraction

import numpy as np

from oracle import KP_DTYPE, WQ_DTYPE

BOUNDS = (0.0, 0.0, 640.0, 480.0)
BEST, SAME_LEVEL, RATIO, INIT = "best", "same_level", "ratio", "init"
INT_MAX = 2**31 - 1
TH_LOW, TH_HIGH = 45, 95
FAR = 200                    # a filler candidate: beyond every threshold used here, and no ratio test fails against it
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)
f32 = np.float32

_BASE = np.random.default_rng(20240611).integers(0, 2, 256).astype(bool)


def pack(bits):
    """The 32-byte descriptor of BASE with the given bit positions flipped."""
    m = _BASE.copy()
    m[np.asarray(bits, np.int64)] ^= True
    return np.packbits(m)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def accepts(rule, best, second, l1, l2, th, ratio):
    """The reference's acceptance of a (best, second) pair, second = None when the best candidate is alone.
    BEST        bestDist <= th                                                             (:1634, :1766, :585)
    SAME_LEVEL  bestDist <= th, not (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2); alone: level2 = -1  (:119-122)
    RATIO       bestDist1 <= th && (float)bestDist1 < mfNNratio * (float)bestDist2; alone: bestDist2 = 256             (:429-431, :799-801)
    INIT        bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio; alone: bestDist2 = INT_MAX             (:674-676)
    The products are float32 (a float ratio times a converted int)."""
    r = f32(ratio)
    if best > th:
        return False
    if rule == BEST:
        return True
    if rule == SAME_LEVEL:
        return not (second is not None and l1 == l2 and f32(best) > r * f32(second))
    if rule == RATIO:
        return bool(f32(best) < r * f32(256 if second is None else second))
    return bool(f32(best) < f32(INT_MAX if second is None else second) * r)


@functools.lru_cache(maxsize=None)
def ratio_triples(rule, th, ratio, limit=3):
    """(best, second, tag) pairs around the ratio test of `rule`: where the float32 product decides differently from the double
    product of the same float ratio (f32_vs_double) or from exact arithmetic with the decimal ratio (f32_vs_exact), where
    best = ratio * second exactly (equal), one beside it (beside), and one plain pass and fail."""
    r32, rq = f32(ratio), Fraction(str(ratio))
    out, seen = [], {}
    def add(b, s, tag):
        if seen.setdefault(tag, 0) < limit and 1 <= b <= s and (b, s, tag) not in out:
            out.append((b, s, tag)); seen[tag] += 1
    for s in range(2, 140):
        for b in range(1, min(th, s) + 1):
            if rule == SAME_LEVEL:
                d32, d64, dq = f32(b) > r32 * f32(s), float(b) > float(r32) * s, Fraction(b) > rq * s
            else:
                d32, d64, dq = f32(b) < r32 * f32(s), float(b) < float(r32) * s, Fraction(b) < rq * s
            if bool(d32) != d64: add(b, s, "f32_vs_double")
            if bool(d32) != dq: add(b, s, "f32_vs_exact")
            if Fraction(b) == rq * s:
                add(b, s, "equal"); add(b - 1, s, "beside"); add(b + 1, s, "beside")
    add(5, 40, "plain"); add(30, 31, "plain")
    return out


class Query:
    def __init__(self, T, takes, best, second, free, want, level, angle, dummy, imax):
        self.T, self.takes, self.best, self.second, self.free, self.want = T, takes, best, second, free, want
        self.level, self.angle, self.dummy, self.imax = level, angle, dummy, imax


class Island:
    """Candidates in visiting order and the queries that see exactly them, in call order."""

    def __init__(self, name, tags=(), split=None):
        self.name, self.tags, self.split = name, set(tags) | {name}, split
        self.S, self.level, self.kangle, self.queries = [], [], [], []
        self._next, self._seen = 0, set()
        self._rng = np.random.default_rng(zlib.crc32(name.encode()))

    def cand(self, d, level=0, angle=0.0):
        """A candidate at distance d from a plain query.  While they fit, the bit sets of an island are disjoint (so a query
        that flips part of one set moves away from all the others); after that they are random sets of d bits, all distinct."""
        if d == 256:
            bits = np.arange(256)
        elif self._next + d <= 256:
            bits = np.arange(self._next, self._next + d); self._next += d
        else:
            while True:
                bits = np.sort(self._rng.choice(256, d, replace=False))
                if bits.tobytes() not in self._seen:
                    break
        self._seen.add(bits.tobytes())
        self.S.append(bits); self.level.append(level); self.kangle.append(angle)
        return len(self.S) - 1

    def cands(self, dists, level=0):
        return [self.cand(d, level) for d in dists]

    def query(self, T=(), takes=1, best=None, second=None, free=None, want=None, level=0, angle=0.0, dummy=False, imax=None):
        """T: [(candidate, nbits)]: the query flips the first nbits bits of that candidate's set.  free = (best, second) when
        nothing blocks (default: as declared); imax = the same when 256 is a distance like any other (init_dist = INT_MAX)."""
        bits = np.concatenate([self.S[c][:k] for c, k in T]).astype(np.int64) if T else np.zeros(0, np.int64)
        self.queries.append(Query(bits, takes, best, second, (best, second) if free is None else free, want, level, angle, dummy, imax))
        return self

    def block(self, cs, takes=1):
        """One blocker per listed candidate (distance 0: every rule accepts it, whatever its second is)."""
        for c in cs:
            self.query(T=[(c, len(self.S[c]))], takes=takes, best=c, second=None, want=True)
        return self

    # geometry: per column, how many candidates
    def columns(self):
        return list(self.split) if self.split else [len(self.S)]

    def ncol(self): return len(self.columns())
    def nrow(self): return max(1, max((c + 63) // 64 for c in self.columns()))
    def radius(self): return 5 * max(self.ncol(), self.nrow())


# ---------------------------------------------------------------------------------------------------- the families
def blocked_prefix(I, dists, level=0, takes=1):
    cs = I.cands(dists, level)
    I.block(cs, takes)
    return cs


def threshold_islands(rule, th, ratio):
    out = []
    I = Island("th_eq"); c = I.cand(th); I.query(best=c, want=True); out.append(I)
    I = Island("th_plus1"); c = I.cand(th + 1); I.query(best=c if th < 255 else None, want=False if th < 255 else None); out.append(I)
    # a candidate at 256 is never selected by the projection / BoW rules (dist < bestDist from 256 never fires) but it is a
    # candidate like any other from INT_MAX (SearchForInitialization, search_window(init_dist = INT_MAX))
    I = Island("never_256"); c0 = I.cand(256); c1 = I.cand(min(th, 255))
    I.query(best=c1, second=c0 if rule == INIT else None, want=True, imax=(c1, c0)); out.append(I)
    I = Island("only_256"); c0 = I.cand(256)
    I.query(best=c0 if rule == INIT else None, want=False if rule == INIT else None, imax=(c0, None)); out.append(I)
    return out


def ratio_islands(rule, th, ratio):
    out = []
    if rule == BEST:
        return out
    for b, s, tag in ratio_triples(rule, th, ratio):
        levels = [(0, 0)] if rule != SAME_LEVEL else [(0, 0), (3, 4), (15, 15), (15, 14)]
        for l1, l2 in levels:
            for order in (0, 1):
                I = Island(f"ratio_{tag}_{b}_{s}_l{l1}_{l2}_o{order}", tags=("ratio_" + tag, f"levels_{l1}_{l2}"))
                if order == 0:
                    cb = I.cand(b, l1); cs = I.cand(s, l2)
                else:
                    cs = I.cand(s, l2); cb = I.cand(b, l1)
                if b == s and order == 1:
                    cb, cs = cs, cb         # a tie: the first in visiting order is the best
                I.query(best=cb, second=cs, want=True if (rule == SAME_LEVEL and l1 != l2) else None)
                out.append(I)
    return out


def tie_islands(rule, th, ratio):
    out = []
    I = Island("tie2"); a, b = I.cands([10, 10]); I.query(best=a, second=b, want=rule == BEST); out.append(I)
    I = Island("tie3"); a, b, c = I.cands([10, 10, 10]); I.query(best=a, second=b, want=rule == BEST); out.append(I)
    if rule == SAME_LEVEL:
        I = Island("tie2_levels"); a = I.cand(10, 1); b = I.cand(10, 2); I.query(best=a, second=b, want=True); out.append(I)
    out.append(tie_8_9(0))
    return out


def tie_8_9(extra):
    """Seven taken candidates in front, then two at one distance: the 8th and 9th entry by (distance, position).  The short list
    holds the earlier one.  extra > 0: fillers behind them, for the lists that wave_topk reads back."""
    I = Island(f"tie_8_9_{extra}", tags=("tie_8_9",))
    blocked_prefix(I, range(1, 8))
    a, b = I.cands([20, 20])
    for _ in range(extra):
        I.cand(FAR)
    I.query(best=a, second=b, free=(0, 1))
    return I


def length_island(L, wpos):
    """A list of L candidates, fillers but for the winner (10) at wpos and the runner-up (30) next to it."""
    I = Island(f"len{L}_w{wpos}", tags=(f"len_{L}", "winner_" + ("first" if wpos == 0 else "last" if wpos == L - 1 else str(wpos + 1))))
    rpos = (wpos + 1) % L
    for p in range(L):
        I.cand(10 if p == wpos else (30 if p == rpos else FAR))
    I.query(best=wpos, second=rpos if L > 1 else None, want=True)
    return I


def length_islands(lengths):
    out = []
    for L in lengths:
        for wpos in sorted({0, 7, 8, L - 1}):
            if wpos < L:
                out.append(length_island(L, wpos))
    return out


def step_islands():
    """Window lists of four and of five 64-candidate steps with fewer than 256 entries (two / three columns): k_win_wave builds the
    short list from its registers up to four steps and reads the list back beyond; the winner is the last candidate."""
    out = []
    for name, split in (("steps4", [65, 65]), ("steps5", [65, 65, 1])):
        n = sum(split)
        I = Island(name, split=split)
        for p in range(n):
            I.cand(10 if p == n - 1 else (30 if p == 0 else FAR))
        I.query(best=n - 1, second=0, want=True)
        out.append(I)
    return out


def route_islands(rule, th, ratio):
    """The three routes of select_two.  D7: the distance of the taken short-list entries against which best = 12 FAILS its ratio
    test on one level; P: a second against which it passes."""
    out = []
    # found == 0: all eight short-list entries taken
    I = Island("found0_scan_d7_eq_th")          # d7 = th: the scan must run, and finds the 9th candidate at th
    blocked_prefix(I, list(range(1, 8)) + [th])
    c = I.cand(th); f = I.cand(FAR)
    I.query(best=c, second=f, free=(0, 1), want=True); out.append(I)
    I = Island("found0_noscan_d7_above_th")
    blocked_prefix(I, list(range(1, 8)) + [th + 1])
    c = I.cand(th + 2)
    I.query(best=c, second=None, free=(0, 1), want=False); out.append(I)
    # found == 1
    r = ratio if rule != BEST else 0.6
    pair = RATIO if rule == BEST else rule
    D7 = max(d for d in range(13, 64) if not accepts(pair, 12, d, 0, 0, 255, r))
    P = D7 + 4
    assert not accepts(pair, 12, D7, 0, 0, 255, r) and accepts(pair, 12, P, 0, 0, 255, r) and D7 > 12
    I = Island("found1_best_above_th")
    blocked_prefix(I, [D7] * 7)
    c = I.cand(th + 1); I.cands([FAR, FAR])
    I.query(best=c, second=8, free=(0, 1), want=False); out.append(I)
    I = Island("found1_shortcut_pass")          # best passes against d7: decided without the scan, and as the full rule decides
    c = I.cand(5); blocked_prefix(I, [16] * 7); s = I.cand(40); I.cand(FAR)
    I.query(best=c, second=s, free=(c, 1), want=True); out.append(I)
    for name, sec_d, sec_l, blocked in (("found1_scan_second_other_level", D7, 1, False), ("found1_scan_second_same_level", D7, 0, False),
                                        ("found1_scan_all_blocked", D7, 0, True), ("found1_scan_second_passes", P, 0, False)):
        I = Island(name)
        blocked_prefix(I, [D7] * 7)
        c = I.cand(12)
        s = I.cand(sec_d, 0 if rule == INIT else sec_l)
        if blocked:
            I.block([s])
        else:
            I.cand(FAR)
        I.query(best=c, second=None if blocked else s, free=(c, 0), want=True if blocked or sec_d == P else None)
        out.append(I)
    return out


def claim_island(nclaim, offset):
    """nclaim identical queries behind `offset` queries without candidates: all want candidate 0; the first keeps it, the next
    takes its own second choice, and so on.  (5, 10, 20, 40: every rule accepts each of them for every ratio used here; under
    SearchForInitialization the later ones find candidate 0 recorded at their own distance, which shuts it: :645-646.)"""
    I = Island(f"claim{nclaim}_at{offset}", tags=(f"claim{nclaim}", f"claim_at_{offset}"))
    I.cands([5, 10, 20, 40]); I.cand(FAR)
    for _ in range(offset):
        I.query(dummy=True)
    for k in range(nclaim):
        I.query(best=k, second=k + 1, free=(0, 1), want=True)
    return I


def init_islands(ratio):
    """SearchForInitialization's own coupling: vMatchedDistance."""
    out = []
    I = Island("init_steal")                    # a later query at a strictly lower distance takes the keypoint: one up, one down
    c0 = I.cand(8); c1 = I.cand(30)
    I.query(best=c0, second=c1, want=True)
    I.query(T=[(c0, 3)], best=c0, second=c1, want=True)         # 5 to c0, 33 to c1
    out.append(I)
    I = Island("init_equal")                    # at an equal distance the keypoint is left out: the query goes to its next choice
    c0 = I.cand(8); c1 = I.cand(30)
    I.query(best=c0, second=c1, want=True)
    I.query(best=c1, second=None, want=True)
    out.append(I)
    I = Island("init_left_out_of_second")       # 19 to c1, 20 to c0 (recorded at 8): as a second c0 would fail the ratio test
    c0 = I.cand(8); c1 = I.cand(31)
    I.query(best=c0, second=c1, want=True)
    I.query(T=[(c1, 12)], best=c1, second=None, want=True)
    assert not accepts(INIT, 19, 20, 0, 0, TH_LOW, ratio)
    out.append(I)
    I = Island("init_level0_only")              # a query above level 0 is skipped (:622-623); a keypoint above level 0 is no candidate
    c0 = I.cand(5, level=15); c1 = I.cand(20)
    I.query(level=1, dummy=True)
    I.query(best=c1, second=None, want=True)
    out.append(I)
    return out


def acceptors_island(k):
    """k queries accept one keypoint, each closer than the one before: k - 1 steals, one match.  The fixed point keeps the
    acceptors of a slot in a list of init_c = 7 entries; one more and it gives up for the sequential resolver."""
    I = Island(f"init_acceptors_{k}", tags=("init_acceptors",))
    c0 = I.cand(20); c1 = I.cand(FAR)
    for j in range(k):
        I.query(T=[(c0, 2 * j)] if j else (), best=c0, second=c1, want=True)
    return I


def chain_island(c, lead=0):
    """c identical queries that prefer candidates 0, 1, 2, ... in that order (distances 1, 2, 3, ...; ACCEPT_BEST): query i ends
    on candidate i, one iteration of the fixed point after query i - 1.  lead: queries without candidates in front."""
    I = Island(f"chain_{c}_{lead}", tags=("chain",))
    I.cands(range(1, c + 1))
    for _ in range(lead):
        I.query(dummy=True)
    for k in range(c):
        I.query(best=k, second=None, free=(0, 1) if c > 1 else (0, None), want=True)
    return I


def init_chain_island(c, lead=0):
    """The same dependency for SearchForInitialization with one acceptor per keypoint.  The candidates are a walk s_0, s_1, ...
    of 20 flipped bits a step.  Query 0 is 10 from s_0 (and at least 20 from the rest) and takes it.  Query i >= 1 is half
    way between s_{i-1} and s_i: 10 from each.  While s_{i-1} looks open to it, its best and second tie and it accepts nothing;
    once query i - 1 stands on s_{i-1} at 10 -- not above query i's own 10 -- that keypoint is shut (:645-646) and query i takes
    s_i.  So query i settles one iteration after query i - 1, and no keypoint ever has two acceptors."""
    I = Island(f"init_chain_{c}_{lead}", tags=("init_chain",))
    rng = np.random.default_rng(7)
    cur = np.zeros(256, bool)
    sets, steps = [], []
    for k in range(c):
        step = rng.choice(256, 20, replace=False)
        cur = cur.copy(); cur[step] ^= True
        sets.append(cur); steps.append(step)
    for s_ in sets:
        I.S.append(np.nonzero(s_)[0]); I.level.append(0); I.kangle.append(0.0)
    for _ in range(lead):
        I.query(dummy=True, level=1)
    for i in range(c):
        bits = sets[i].copy()
        if i:
            bits[steps[i][:10]] ^= True
            q = Query(np.nonzero(bits)[0], 1, i, None, (i - 1, i), True, 0, 0.0, False, None)
        else:
            other = np.setdiff1d(np.arange(256), steps[1] if c > 1 else steps[0])
            bits[rng.choice(other, 10, replace=False)] ^= True
            q = Query(np.nonzero(bits)[0], 1, 0, None, (0, None), True, 0, 0.0, False, None)
        I.queries.append(q)
        d = np.array([np.count_nonzero(bits ^ s_) for s_ in sets])
        mine = [i - 1, i] if i else [0]
        assert (d[mine] == 10).all() and (np.delete(d, mine) >= 20).all(), (i, d)
    return I


# ---------------------------------------------------------------------------------------------------- scenes
class Scene:
    """Islands laid out on one frame: keypoints, their descriptors, the queries in call order and, per query, the island, the
    declared (best, second) as keypoint indices and distances.  `common_r`: every window has one radius (SearchForInitialization)."""

    def __init__(self, islands, common_r=False, grid=True):
        self.islands = islands
        R = max(i.radius() for i in islands) if common_r else None
        self.window = R
        x = y = shelf = 0
        kx, ky, kl, ka, kd, self.kp0 = [], [], [], [], [], []
        self.q = []
        for I in islands:
            r = R or I.radius()
            h = r // 10 + 1
            w, ht = I.ncol() + 2 * h, I.nrow() + 2 * h
            if not grid:                    # (the BoW entries: no windows, the positions are not read)
                x = y = 0
            elif x + w > 64:
                x, y, shelf = 0, y + shelf, 0
            assert x + w <= 64 and y + ht <= 48, f"scene does not fit the grid at {I.name}"
            c0, r0 = x + h, y + h
            x += w; shelf = max(shelf, ht)
            self.kp0.append(len(kx))
            col_of, pos_in = [], []
            for ci, cnt in enumerate(I.columns()):
                col_of += [ci] * cnt; pos_in += list(range(cnt))
            assert len(col_of) == len(I.S)
            for j, bits in enumerate(I.S):
                kx.append(10.0 * (c0 + col_of[j]) - 4.0 + 0.125 * (pos_in[j] % 64)); ky.append(10.0 * (r0 + pos_in[j] // 64))
                kl.append(I.level[j]); ka.append(I.kangle[j]); kd.append(pack(bits))
            u, v = 10.0 * c0 + 5.0 * (I.ncol() - 1), 10.0 * r0 + 5.0 * (I.nrow() - 1)
            for qi, Q in enumerate(I.queries):
                self.q.append((I, Q, u, v, float(r), pack(Q.T) if not Q.dummy or len(Q.T) else pack(np.arange(256))))
        n = len(kx)
        self.kps = np.zeros(n, KP_DTYPE)
        self.kps["x"], self.kps["y"], self.kps["octave"], self.kps["angle"] = kx, ky, kl, ka
        self.kps["size"] = 31.0
        self.desc = np.stack(kd) if n else np.zeros((0, 32), np.uint8)
        self.nq = len(self.q)
        self.qdesc = np.stack([t[5] for t in self.q])
        self.qangle = np.array([t[1].angle for t in self.q], np.float32)
        self.island_of = [t[0] for t in self.q]
        self.base_of = []
        for I, k0 in zip(islands, self.kp0):
            self.base_of += [k0] * len(I.queries)

    # ---- the queries of each entry
    def windows(self):
        """SearchByProjection-family / window / fuse queries: levels [0, 15]; a dummy has r = -1 (no candidates)."""
        q = np.zeros(self.nq, WQ_DTYPE)
        for i, (I, Q, u, v, r, _) in enumerate(self.q):
            q[i] = (u, v, -1.0 if Q.dummy else r, 0.0, 0, 15)
        return q

    def takes(self, on=1):
        return np.array([t[1].takes if on else 0 for t in self.q], np.uint8)

    def init_queries(self):
        """F1 of SearchForInitialization: keypoints (octave 0; a dummy: its level, or 1), vbPrevMatched = the island's centre."""
        k1 = np.zeros(self.nq, KP_DTYPE); prev = np.zeros((self.nq, 2), np.float32)
        for i, (I, Q, u, v, r, _) in enumerate(self.q):
            k1[i]["x"], k1[i]["y"], k1[i]["angle"], k1[i]["size"] = u, v, Q.angle, 31.0
            k1[i]["octave"] = Q.level if not Q.dummy else max(Q.level, 1)
            prev[i] = (u, v)
        return k1, prev

    def bow(self, valid1=None, valid2=None):
        """Both FeatureVectors: island k is node 10 + 3 k on both sides; set 1 = the queries, set 2 = the keypoints."""
        nodes = np.array([10 + 3 * k for k in range(len(self.islands))], np.int32)
        off1 = np.cumsum([0] + [len(I.queries) for I in self.islands]).astype(np.int32)
        off2 = np.cumsum([0] + [len(I.S) for I in self.islands]).astype(np.int32)
        fv1 = (nodes, off1, np.arange(self.nq, dtype=np.int32))
        fv2 = (nodes, off2, np.arange(len(self.kps), dtype=np.int32))
        return fv1, fv2

    # ---- expectations
    def _pair(self, i, which):
        """(best keypoint, best distance, best level, second distance or None, second level) of query i as declared."""
        I, Q = self.q[i][0], self.q[i][1]
        b, s = {"taken": (Q.best, Q.second), "free": Q.free, "imax": Q.imax if Q.imax is not None else Q.free}[which]
        if Q.dummy and which != "taken":
            b = s = None
        if b is None:
            return None
        k0 = self.base_of[i]
        db = hamming(self.qdesc[i], self.desc[k0 + b])
        ds = hamming(self.qdesc[i], self.desc[k0 + s]) if s is not None else None
        return k0 + b, db, I.level[b], ds, (I.level[s] if s is not None else -1)

    def expect(self, rule, th, ratio, takes=1):
        """match_q [nq] (the accepted keypoint or -1), as each coupled entry reports it before steals and the rotation check."""
        which = "taken" if takes else "free"
        mq = np.full(self.nq, -1, np.int32)
        for i in range(self.nq):
            Q = self.q[i][1]
            p = self._pair(i, which)
            if p is None:
                continue
            ok = accepts(rule, p[1], p[3], p[2], p[4], th, ratio)
            if Q.want is not None and which == "taken":
                assert ok == Q.want, (self.island_of[i].name, rule, th, ratio, p)
            if ok:
                mq[i] = p[0]
        return mq

    def expect_projection(self, rule, th, ratio, takes=1):
        """(match_kp, match_q, nmatches) of the projection family without the rotation check: the last accepted query of a slot."""
        mq = self.expect(rule, th, ratio, takes)
        mk = np.full(len(self.kps), -1, np.int32)
        for i in np.nonzero(mq >= 0)[0]:
            mk[mq[i]] = i
        return mk, mq, int((mq >= 0).sum())

    def expect_init(self, ratio):
        """(vnMatches12, nmatches) without the rotation check: an acceptor stands until a later one accepts the same keypoint."""
        acc = self.expect(INIT, TH_LOW, ratio)
        m12 = acc.copy()
        for i in np.nonzero(acc >= 0)[0]:
            if (acc[i + 1:] == acc[i]).any():
                m12[i] = -1
        return m12, int((m12 >= 0).sum()), acc

    def expect_bow(self, kf_kf, ratio):
        """(match12, match21, nmatches) without the rotation check."""
        m12 = self.expect(RATIO, TH_LOW - 1 if kf_kf else TH_LOW, ratio)
        m21 = np.full(len(self.kps), -1, np.int32)
        for i in np.nonzero(m12 >= 0)[0]:
            assert m21[m12[i]] < 0
            m21[m12[i]] = i
        return m12, m21, int((m12 >= 0).sum())

    def expect_window(self, init_dist):
        """(best, best_level, second, second_level, idx) of the uncoupled search."""
        out = [np.full(self.nq, v, np.int32) for v in (init_dist, -1, init_dist, -1, -1)]
        for i in range(self.nq):
            p = self._pair(i, "imax" if init_dist > 256 else "free")
            if p is None:
                continue
            out[0][i], out[1][i], out[4][i] = p[1], p[2], p[0]
            if p[3] is not None:
                out[2][i], out[3][i] = p[3], p[4]
        return tuple(out)

    def tags(self):
        t = set()
        for I in self.islands:
            t |= I.tags
        return t


SHORT_LENGTHS = (1, 8, 9, 64, 65, 256)
LONG_LENGTHS = (257, 300)


def core_islands(rule, th, ratio):
    """Everything that fits a list region: one call on the strided route."""
    out = threshold_islands(rule, th, ratio)
    if th <= TH_HIGH:
        out += ratio_islands(rule, th, ratio) + tie_islands(rule, th, ratio) + route_islands(rule, th, ratio)
        out += [claim_island(2, 0), claim_island(3, 0)]
    return out


def long_islands():
    """Lists beyond the projection family's region of 256 entries: the call repeats on the exact count / scan / fill route, and
    wave_topk reads lists of more than 256 entries back round by round."""
    I = Island("len257_with_256"); I.cand(256)
    for p in range(256):
        I.cand(10 if p == 100 else (30 if p == 3 else FAR))
    I.query(best=101, second=4, want=True, imax=(101, 4))
    return length_islands(LONG_LENGTHS) + [tie_8_9(300), I]


# every tag a scene family must have produced by the time tests/test_cpu_selection.py ends (with the rule it ran under in front)
REQUIRED = {
    "th_eq", "th_plus1", "never_256", "only_256", "tie2", "tie3", "tie_8_9", "ratio_f32_vs_double", "ratio_equal", "ratio_beside",
    "ratio_plain", "found0_scan_d7_eq_th", "found0_noscan_d7_above_th", "found1_best_above_th", "found1_shortcut_pass",
    "found1_scan_second_other_level", "found1_scan_second_same_level", "found1_scan_all_blocked", "found1_scan_second_passes",
    "claim2", "claim3",
}


# ---------------------------------------------------------------------------------------------------- the catalogue
PROJECTION_RULES = [(BEST, TH_LOW, 0.6), (BEST, TH_HIGH, 0.6), (BEST, 70, 0.6), (BEST, 255, 0.6), (SAME_LEVEL, TH_LOW, 0.6), (SAME_LEVEL, 70, 0.7)] + \
                   [(SAME_LEVEL, TH_HIGH, r) for r in RATIOS]
# (the list-length scenes do not depend on the threshold or the ratio: once per rule)
PROJECTION_SCENES = [(*r, "core") for r in PROJECTION_RULES] + [(rule, TH_HIGH, 0.6, k) for rule in (BEST, SAME_LEVEL) for k in ("lengths", "long")]
INIT_SCENES = [("core", r) for r in RATIOS] + [("lengths", 0.9), ("long", 0.9)]
CLAIM_OFFSETS = (62, 63, 64, 65)        # the claimers start at that query of the call (or of the BoW node): either side of a 64-query batch


@functools.lru_cache(maxsize=None)
def scene(kind, rule=BEST, th=TH_HIGH, ratio=0.6, arg=0):
    """kind: core / lengths / long / claims / chain / many / init_lists / init_acceptors / init_chain / init_many / bow."""
    init = rule == INIT
    if kind == "core":
        return Scene(core_islands(rule, th, ratio) + (init_islands(ratio) if init else []), common_r=init)
    if kind == "lengths":
        return Scene(length_islands(SHORT_LENGTHS) + step_islands(), common_r=init)
    if kind == "long":
        return Scene(long_islands(), common_r=init)
    if kind == "long_plain":            # ... without the blockers (the uncoupled searches)
        return Scene([I for I in long_islands() if "tie_8_9" not in I.tags])
    if kind == "claims":
        return Scene([claim_island(n, arg) for n in (2, 3)], common_r=init)
    if kind == "chain":                 # arg queries in one dependency chain
        return Scene([init_chain_island(arg) if init else chain_island(arg)], common_r=init)
    if kind == "many":                  # arg queries over 16 keypoints, the last 16 of them a chain: 2048 fit the fixed point's registers
        return Scene([init_chain_island(16, arg - 16) if init else chain_island(16, arg - 16)], common_r=init)
    if kind == "init_lists":            # either side of SearchForInitialization's list region of 1024 entries
        return Scene([length_island(1024, 0), length_island(1024, 1023)] if arg == 1024 else [length_island(1025, 1024), length_island(1024, 8)],
                     common_r=True)
    if kind == "init_acceptors":
        return Scene([acceptors_island(arg)], common_r=True)
    if kind == "bow":                   # no grid: every list length in one call
        return Scene(core_islands(RATIO, th, ratio) + length_islands(SHORT_LENGTHS + LONG_LENGTHS) + [tie_8_9(300)] +
                     [claim_island(n, off) for n in (2, 3) for off in CLAIM_OFFSETS], grid=False)
    if kind == "window":                # the uncoupled searches: plain queries only
        return Scene(threshold_islands(BEST, TH_LOW, 0.6) + ratio_islands(SAME_LEVEL, TH_HIGH, 0.7) + tie_islands(SAME_LEVEL, TH_HIGH, 0.7)[:3] +
                     [claim_island(3, 2)])
    raise ValueError(kind)


def rotation_scene(tip):
    """SearchForInitialization: a stolen match still counts in the rotation histogram (:684-693 push it, nothing takes it out).
    Query angle 0 -> bin 0, 30 -> bin 1 (keypoint angles 0).  ComputeThreeMaxima drops bin 1 when its count < 0.1f * bin 0's.
    tip = "keep": bin 0 = 20 matches, bin 1 = one standing match + the match it stole: 2 < 2.0f is false, bin 1 stays
                  (counted without the stolen one: 1 < 2.0f, the standing match would go).
    tip = "drop": bin 0 = 9 matches + a stealer + the match it stole = 11, bin 1 = 1: 1 < 1.1f, bin 1 goes
                  (without the stolen one: 1 < 1.0f is false, it would stay).
    Returns (Scene, expected vnMatches12, expected nmatches)."""
    keep = tip == "keep"
    isl = []
    for k in range(20 if keep else 9):
        I = Island(f"rot_pair_{k}"); c = I.cand(5); I.query(best=c, want=True, angle=0.0); isl.append(I)
    a = 30.0 if keep else 0.0
    I = Island("rot_steal"); c0 = I.cand(8); c1 = I.cand(30)
    I.query(best=c0, second=c1, want=True, angle=a)
    I.query(T=[(c0, 3)], best=c0, second=c1, want=True, angle=a)
    isl.append(I)
    if not keep:
        I = Island("rot_bin1"); c = I.cand(5); I.query(best=c, want=True, angle=30.0); isl.append(I)
    sc = Scene(isl, common_r=True)
    m12, nm, _ = sc.expect_init(0.9)
    if not keep:
        assert m12[-1] >= 0
        m12[-1] = -1; nm -= 1
    assert nm == (21 if keep else 10)
    return sc, m12, nm


def bow_special(kf_kf):
    """Nodes of the two FeatureVectors that the co-iteration must handle: one member each side (node 5), a node of the first set
    only (7), of the second only (8), a node whose queries are all invalid (9), a node whose members are all invalid in the
    second set (11: the KeyFrame form skips them, the Frame form has no such flag) and one with its nearest member invalid (12).
    Returns the arguments of SearchByBoW and the expected (match12, match21, nmatches)."""
    I = Island("bow_special")
    k = [I.cand(d) for d in (10, 7, 6, 5, 5, 20)]          # keypoints 0..5 of the second set
    d2 = np.stack([pack(I.S[j]) for j in k])
    d1 = np.stack([pack(np.zeros(0, np.int64))] * 2 + [pack(I.S[2])] + [pack(np.zeros(0, np.int64))] * 2)   # queries 0..4 (2: distance 0 to keypoint 2)
    fv1 = (np.array([5, 7, 9, 11, 12], np.int32), np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32))
    fv2 = (np.array([5, 8, 9, 11, 12], np.int32), np.array([0, 1, 2, 3, 4, 6], np.int32), np.arange(6, dtype=np.int32))
    valid1 = np.array([1, 1, 0, 1, 1], np.uint8)
    valid2 = np.array([1, 1, 1, 0, 0, 1], np.uint8)
    m12 = np.array([0, -1, -1, -1, 5], np.int32) if kf_kf else np.array([0, -1, -1, 3, 4], np.int32)
    m21 = np.full(6, -1, np.int32)
    m21[m12[m12 >= 0]] = np.nonzero(m12 >= 0)[0]
    return dict(fv1=fv1, valid1=valid1, desc1=d1, fv2=fv2, valid2=valid2, desc2=d2), (m12, m21, int((m12 >= 0).sum()))
