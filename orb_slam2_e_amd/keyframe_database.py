"""KeyFrameDatabase (src/KeyFrameDatabase.cc:40-309) over the device store of orbm_kfdb.hip.  A keyframe is known by the SLOT add()
returns (ascending in the order of add, restarting at 0 after clear()).  Both detect methods are three stages:

  1. ONE orbm_kfdb_query: per slot the number of words shared with the query, the query index of the first shared word and the
     float L1 score (the only stage that needs the device);
  2. a pure function over those three arrays and the per-slot fields that persist across queries (SlotFields): the list of
     keyframes sharing words in the reference's order -- (first shared word's position in the query, then slot) --, the loop
     form's connected keyframes, maxCommonWords, the int(max * 0.8f) cut, the minScore filter, and the fields written exactly where
     the reference writes them;
  3. the covisibility fold and the 0.75 cut in np.float32 arithmetic; best_covisibles(slot) is the caller's
     GetBestCovisibilityKeyFrames(10) in slots (a neighbour that was never added to the database has no slot and is left out:
     no query can have listed it).

Stages 2 and 3 are module functions and need no device.  The reference never initialises mLoopScore / mRelocScore; here they
start at 0.0f.  A query id of 0 lists nobody, as in the reference (mnLoopQuery / mnRelocQuery start at 0)."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr as _p

F32 = np.float32


class SlotFields:
    """mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore of every slot handed out (erased ones too:
    the covisibility graph may still name them)."""
    NAMES = ("loop_query", "loop_words", "loop_score", "reloc_query", "reloc_words", "reloc_score")
    TYPES = (np.int64, np.int32, np.float32, np.int64, np.int32, np.float32)

    def __init__(self):
        self.n = 0
        for name, t in zip(self.NAMES, self.TYPES):
            setattr(self, "_" + name, np.zeros(64, t))

    def resize(self, n):
        """n slots; new ones start at 0 / 0 / 0.0f"""
        cap = len(self._loop_query)
        if n > cap:
            for name, t in zip(self.NAMES, self.TYPES):
                a = np.zeros(max(n, 2 * cap), t)
                a[:self.n] = getattr(self, "_" + name)[:self.n]
                setattr(self, "_" + name, a)
        for name in self.NAMES:
            getattr(self, "_" + name)[min(n, self.n):max(n, self.n)] = 0
        self.n = n

    def arrays(self):
        return tuple(getattr(self, "_" + name)[:self.n] for name in self.NAMES)


for _name in SlotFields.NAMES:
    setattr(SlotFields, _name, property(lambda self, _n="_" + _name: getattr(self, _n)[:self.n]))


def bow_arrays(bow):
    """{word: value} -> (ids ascending int32, values float64): the BowVector as std::map iterates it"""
    words = np.array(sorted(bow), np.int32)
    return words, np.array([bow[int(w)] for w in words], np.float64)


def min_common_words(max_common):
    return int(F32(max_common) * F32(0.8))           # int minCommonWords = maxCommonWords*0.8f;


def sharing_order(common, first):
    """slots that share a word with the query, in the order the reference's walk meets them first"""
    s = np.nonzero(np.asarray(common) > 0)[0]
    return s[np.lexsort((s, np.asarray(first)[s]))]


def loop_stage2(fields, common, first, score, query_id, connected_slots, min_score):
    """KeyFrameDatabase.cc:86-139.  Returns (scored, min_common): scored = [(score, slot)] of the keyframes that pass the word cut
    and reach min_score, in list order."""
    connected = set(int(c) for c in connected_slots)
    lq, lw, ls = fields.loop_query, fields.loop_words, fields.loop_score
    listed = []
    for s in sharing_order(common, first):
        s = int(s)
        if lq[s] != query_id:
            if s in connected:
                lw[s] = 1                            # reset to 0 at every meeting, then incremented
            else:
                lq[s] = query_id
                lw[s] = common[s]
                listed.append(s)
        else:
            lw[s] += common[s]                       # listed by an earlier query of this id: not listed again, still counted
    if not listed:
        return [], 0
    min_common = min_common_words(max(int(lw[s]) for s in listed))
    min_score = F32(min_score)
    scored = []
    for s in listed:
        if lw[s] > min_common:
            ls[s] = score[s]
            if ls[s] >= min_score:
                scored.append((F32(score[s]), s))
    return scored, min_common


def reloc_stage2(fields, common, first, score, query_id):
    """KeyFrameDatabase.cc:207-253"""
    rq, rw, rs = fields.reloc_query, fields.reloc_words, fields.reloc_score
    listed = []
    for s in sharing_order(common, first):
        s = int(s)
        if rq[s] != query_id:
            rq[s] = query_id
            rw[s] = common[s]
            listed.append(s)
        else:
            rw[s] += common[s]
    if not listed:
        return [], 0
    min_common = min_common_words(max(int(rw[s]) for s in listed))
    scored = []
    for s in listed:
        if rw[s] > min_common:
            rs[s] = score[s]
            scored.append((F32(score[s]), s))
    return scored, min_common


def _retain(acc_list, best_acc):
    retain = F32(F32(0.75) * best_acc)
    out, seen = [], set()
    for acc, s in acc_list:
        if acc > retain and s not in seen:
            out.append(s)
            seen.add(s)
    return out


def loop_stage3(fields, scored, min_common, query_id, min_score, best_covisibles):
    """KeyFrameDatabase.cc:141-196"""
    if not scored:
        return []
    lq, lw, ls = fields.loop_query, fields.loop_words, fields.loop_score
    acc_list = []
    best_acc = F32(min_score)
    for si, s in scored:
        best, acc, best_slot = si, si, s
        for s2 in best_covisibles(s):
            if lq[s2] == query_id and lw[s2] > min_common:
                acc = F32(acc + ls[s2])
                if ls[s2] > best:
                    best_slot, best = int(s2), ls[s2]
        acc_list.append((acc, best_slot))
        if acc > best_acc:
            best_acc = acc
    return _retain(acc_list, best_acc)


def reloc_stage3(fields, scored, query_id, best_covisibles):
    """KeyFrameDatabase.cc:255-308"""
    if not scored:
        return []
    rq, rs = fields.reloc_query, fields.reloc_score
    acc_list = []
    best_acc = F32(0.0)
    for si, s in scored:
        best, acc, best_slot = si, si, s
        for s2 in best_covisibles(s):
            if rq[s2] != query_id:
                continue
            acc = F32(acc + rs[s2])                  # also of a neighbour this query did not score: the reference's stale value
            if rs[s2] > best:
                best_slot, best = int(s2), rs[s2]
        acc_list.append((acc, best_slot))
        if acc > best_acc:
            best_acc = acc
    return _retain(acc_list, best_acc)


class KeyFrameDatabase:
    def __init__(self, nwords):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.orbm_kfdb_create(int(nwords), C.byref(self._h)))
        self.fields = SlotFields()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.orbm_kfdb_destroy(h)
            self._h = None

    def add(self, bow):
        words, values = bow_arrays(bow)
        slot = C.c_int(-1)
        check(self._L.orbm_kfdb_add(self._h, _p(words), _p(values), len(words), C.byref(slot)))
        self.fields.resize(slot.value + 1)
        return slot.value

    def erase(self, slot):
        check(self._L.orbm_kfdb_erase(self._h, int(slot)))

    def clear(self):
        check(self._L.orbm_kfdb_clear(self._h))
        self.fields.resize(0)

    def size(self):
        """(live keyframes, slots handed out since the last clear)"""
        live, slots = C.c_int(0), C.c_int(0)
        check(self._L.orbm_kfdb_size(self._h, C.byref(live), C.byref(slots)))
        return live.value, slots.value

    def reallocations(self):
        return self._L.orbm_debug_kfdb_reallocs(self._h)

    def last_waits(self):
        return self._L.orbm_debug_last_kfdb_waits()

    def query(self, bow):
        """(common, first, score), one entry per slot (orbm_kfdb_query)"""
        words, values = bow_arrays(bow)
        n = self.size()[1]
        common = np.empty(n, np.int32); first = np.empty(n, np.int32); score = np.empty(n, np.float32)
        check(self._L.orbm_kfdb_query(self._h, _p(words), _p(values), len(words), _p(common), _p(first), _p(score)))
        return common, first, score

    def score(self, bow, slots):
        """float scores of the query against the listed live slots: DetectLoop's minScore loop (LoopClosing.cc:127-138)"""
        words, values = bow_arrays(bow)
        slots = np.ascontiguousarray(slots, np.int32)
        out = np.empty(len(slots), np.float32)
        check(self._L.orbm_kfdb_score(self._h, _p(words), _p(values), len(words), _p(slots), len(slots), _p(out)))
        return out

    def detect_loop_candidates(self, bow, query_id, connected_slots, min_score, best_covisibles):
        common, first, score = self.query(bow)
        scored, min_common = loop_stage2(self.fields, common, first, score, query_id, connected_slots, min_score)
        return loop_stage3(self.fields, scored, min_common, query_id, min_score, best_covisibles)

    def detect_relocalization_candidates(self, bow, query_id, best_covisibles):
        common, first, score = self.query(bow)
        scored, _ = reloc_stage2(self.fields, common, first, score, query_id)
        return reloc_stage3(self.fields, scored, query_id, best_covisibles)
