"""KeyFrameDatabase as the reference runs it, restated in plain Python from src/KeyFrameDatabase.cc:40-309 and
Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68: the inverted file as one list of keyframes per word, the per-keyframe fields that
persist across queries, and L1Scoring::score with Python floats (IEEE doubles) cast to np.float32 where the reference assigns to a
float.  A keyframe is known by its SLOT: the number add() gave it, ascending in the order of add and restarting at 0 after clear().

Two things the reference leaves open are pinned here: mLoopScore / mRelocScore, which it never initialises, start at 0.0f; and
clear() also forgets the keyframes (the reference keeps the objects, but nothing reaches them through the database any more)."""
import bisect

import numpy as np

F32 = np.float32


class KF:
    def __init__(self, slot, bow):
        self.slot = slot
        self.words = sorted(bow)                     # std::map order
        self.values = [float(bow[w]) for w in self.words]
        self.alive = True
        self.mnLoopQuery = 0; self.mnLoopWords = 0; self.mLoopScore = F32(0.0)       # KeyFrame.cc:38 (scores: pinned)
        self.mnRelocQuery = 0; self.mnRelocWords = 0; self.mRelocScore = F32(0.0)


def l1_score(w1, v1, w2, v2):
    """ScoringObject.cpp:23-68 over two BowVectors given as ascending ids and values: the co-iteration with lower_bound, the double
    sum in ascending word id, -score / 2.0 (-0.0 when nothing is shared)."""
    a = b = 0
    score = 0.0
    while a < len(w1) and b < len(w2):
        if w1[a] == w2[b]:
            vi, wi = v1[a], v2[b]
            score += abs(vi - wi) - abs(vi) - abs(wi)
            a += 1; b += 1
        elif w1[a] < w2[b]:
            a = bisect.bisect_left(w1, w2[b], a)
        else:
            b = bisect.bisect_left(w2, w1[a], b)
    return -score / 2.0


def min_common_words(max_common):
    return int(F32(max_common) * F32(0.8))           # int minCommonWords = maxCommonWords*0.8f;  (:120, :235)


class ReferenceDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.clear()

    # ---- :40-73
    def add(self, bow):
        kf = KF(len(self.kfs), bow)
        assert all(0 <= w < self.nwords for w in kf.words)
        self.kfs.append(kf)
        for w in kf.words:
            self.inverted.setdefault(w, []).append(kf)
        return kf.slot

    def erase(self, slot):
        kf = self.kfs[slot]
        assert kf.alive
        for w in kf.words:
            self.inverted[w].remove(kf)              # the others keep their order
        kf.alive = False

    def clear(self):
        self.inverted = {}
        self.kfs = []

    def score(self, bow, slots):
        """LoopClosing.cc:127-138: float score = mpORBVocabulary->score(CurrentBowVec, BowVec)"""
        qw = sorted(bow); qv = [float(bow[w]) for w in qw]
        return np.array([F32(l1_score(qw, qv, self.kfs[s].words, self.kfs[s].values)) for s in slots], np.float32)

    def shared(self, bow):
        """What a query finds, without touching a field: per slot the number of shared words, the query index of the first one
        and the score -- the contract of orbm_kfdb_query (dead slot: -1, -1, +0.0f)."""
        n = len(self.kfs)
        common = np.zeros(n, np.int32); first = np.full(n, -1, np.int32); score = np.zeros(n, np.float32)
        qw = sorted(bow); qv = [float(bow[w]) for w in qw]
        for i, w in enumerate(qw):
            for kf in self.inverted.get(w, ()):
                if common[kf.slot] == 0:
                    first[kf.slot] = i
                common[kf.slot] += 1
        for kf in self.kfs:
            if kf.alive:
                score[kf.slot] = F32(l1_score(qw, qv, kf.words, kf.values))
            else:
                common[kf.slot] = -1
        return common, first, score

    # ---- :76-197
    def detect_loop_candidates(self, bow, query_id, connected_slots, min_score, best_covisibles):
        qw = sorted(bow); qv = [float(bow[w]) for w in qw]
        connected = set(connected_slots)
        min_score = F32(min_score)
        sharing = []
        for w in qw:
            for kf in self.inverted.get(w, ()):
                if kf.mnLoopQuery != query_id:
                    kf.mnLoopWords = 0
                    if kf.slot not in connected:
                        kf.mnLoopQuery = query_id
                        sharing.append(kf)
                kf.mnLoopWords += 1
        self.last_sharing = [kf.slot for kf in sharing]
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.mnLoopWords > max_common:
                max_common = kf.mnLoopWords
        min_common = min_common_words(max_common)
        scored = []
        for kf in sharing:
            if kf.mnLoopWords > min_common:
                si = F32(l1_score(qw, qv, kf.words, kf.values))
                kf.mLoopScore = si
                if si >= min_score:
                    scored.append((si, kf))
        if not scored:
            return []
        acc_list = []
        best_acc = min_score
        for si, kf in scored:
            best, acc, best_kf = si, si, kf
            for s2 in best_covisibles(kf.slot):
                kf2 = self.kfs[s2]
                if kf2.mnLoopQuery == query_id and kf2.mnLoopWords > min_common:
                    acc = F32(acc + kf2.mLoopScore)
                    if kf2.mLoopScore > best:
                        best_kf = kf2
                        best = kf2.mLoopScore
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_list, best_acc)

    # ---- :199-309
    def detect_relocalization_candidates(self, bow, query_id, best_covisibles):
        qw = sorted(bow); qv = [float(bow[w]) for w in qw]
        sharing = []
        for w in qw:
            for kf in self.inverted.get(w, ()):
                if kf.mnRelocQuery != query_id:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = query_id
                    sharing.append(kf)
                kf.mnRelocWords += 1
        self.last_sharing = [kf.slot for kf in sharing]
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.mnRelocWords > max_common:
                max_common = kf.mnRelocWords
        min_common = min_common_words(max_common)
        scored = []
        for kf in sharing:
            if kf.mnRelocWords > min_common:
                si = F32(l1_score(qw, qv, kf.words, kf.values))
                kf.mRelocScore = si
                scored.append((si, kf))
        if not scored:
            return []
        acc_list = []
        best_acc = F32(0.0)
        for si, kf in scored:
            best, acc, best_kf = si, si, kf
            for s2 in best_covisibles(kf.slot):
                kf2 = self.kfs[s2]
                if kf2.mnRelocQuery != query_id:
                    continue
                acc = F32(acc + kf2.mRelocScore)          # (also of a neighbour this query did not score: a stale value)
                if kf2.mRelocScore > best:
                    best_kf = kf2
                    best = kf2.mRelocScore
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_list, best_acc)

    @staticmethod
    def _retain(acc_list, best_acc):
        retain = F32(F32(0.75) * best_acc)
        out, seen = [], set()
        for acc, kf in acc_list:
            if acc > retain and kf.slot not in seen:
                out.append(kf.slot)
                seen.add(kf.slot)
        return out

    def fields(self):
        """the six persistent fields of every slot: (loop query, loop words, loop score, reloc query, reloc words, reloc score)"""
        k = self.kfs
        return (np.array([f.mnLoopQuery for f in k], np.int64), np.array([f.mnLoopWords for f in k], np.int32),
                np.array([f.mLoopScore for f in k], np.float32), np.array([f.mnRelocQuery for f in k], np.int64),
                np.array([f.mnRelocWords for f in k], np.int32), np.array([f.mRelocScore for f in k], np.float32))
