"""Seeded databases and queries for the KeyFrameDatabase tests, and the plumbing of tests/kfdb_oracle.cc (build, case text, parsed
output).  Words are drawn from "places": every place owns a pool of words, a keyframe of a place takes a chosen fraction of its
words from that pool and the rest from the whole vocabulary, so a query of a place overlaps that place's keyframes by a controlled
amount and the others by a little.  Values are positive and L1-normalised in std::map order, as vocabulary.assemble_bow leaves
them."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def normalised(words, weights):
    """{word: value} with sum |value| = 1, the norm summed in ascending word id (BowVector::normalize)"""
    order = np.argsort(words)
    words, weights = np.asarray(words)[order], np.asarray(weights, np.float64)[order]
    norm = 0.0
    for v in weights:
        norm += abs(float(v))
    return {int(w): float(v) / norm for w, v in zip(words, weights)}


def bow_of(rng, words):
    words = np.unique(np.asarray(words, np.int64))
    return normalised(words, rng.uniform(0.05, 4.0, len(words))) if len(words) else {}


class Places:
    def __init__(self, rng, nwords, nplaces, pool):
        self.rng, self.nwords = rng, nwords
        self.pools = [rng.choice(nwords, min(pool, nwords), replace=False) for _ in range(nplaces)]

    def bow(self, place, n, share):
        """n words (fewer where draws coincide), about share * n of them from the place's pool"""
        k = min(int(round(share * n)), len(self.pools[place]))
        own = self.rng.choice(self.pools[place], k, replace=False)
        rest = self.rng.integers(0, self.nwords, max(n - k, 0))
        return bow_of(self.rng, np.concatenate([own, rest]))


def sequence(seed, nwords=1000, nkf=40, nqueries=8, nplaces=4, words=60, clear_at=None):
    """Operations over one database, interleaved: ("add", bow, best) -- best = up to 10 earlier slots, the covisibility list of the
    new slot --, ("erase", slot), ("clear",), ("loop", bow, id, connected, min_score), ("reloc", bow, id).  Query ids repeat now
    and then and one is 0, so the fields left by an earlier query of the same id are met."""
    rng = np.random.default_rng(seed)
    pl = Places(rng, nwords, nplaces, 2 * words)
    ops, alive, nslots = [], [], 0
    ids = []
    per_query = max(nkf // max(nqueries, 1), 1)
    for q in range(nqueries):
        for _ in range(per_query):
            best = [int(s) for s in rng.choice(nslots, min(nslots, int(rng.integers(0, 11))), replace=False)] if nslots else []
            ops.append(("add", pl.bow(int(rng.integers(nplaces)), int(rng.integers(words // 2, words + 1)), float(rng.uniform(0.3, 0.95))), best))
            alive.append(nslots); nslots += 1
        for _ in range(int(rng.integers(0, 3))):
            if len(alive) > 3:
                ops.append(("erase", alive.pop(int(rng.integers(len(alive))))))
        qid = 0 if q == 2 else (ids[int(rng.integers(len(ids)))] if ids and rng.random() < 0.25 else 10 + q)
        ids.append(qid)
        qbow = pl.bow(int(rng.integers(nplaces)), words, 0.9)
        if q % 2 == 0:
            connected = [int(s) for s in rng.choice(nslots, min(nslots, 4), replace=False)]
            ops.append(("loop", qbow, qid, connected, float(rng.uniform(0.0, 0.15))))
        else:
            ops.append(("reloc", qbow, qid))
        if clear_at is not None and q == clear_at:
            ops.append(("clear",))
            alive, nslots = [], 0
    return ops


# ------------------------------------------------------------------------------------------------------- tests/kfdb_oracle.cc
def build_oracle(out_dir, flags=("-O2", "-ffp-contract=off")):
    exe = os.path.join(str(out_dir), "kfdb_oracle")
    subprocess.check_call(["g++", "-std=c++17", *flags, os.path.join(HERE, "kfdb_oracle.cc"), "-o", exe])
    return exe


def bow_text(bow):
    return " ".join([str(len(bow))] + [f"{w} {float(bow[w]).hex()}" for w in sorted(bow)])


def case_text(nwords, ops, dump_each_query=True):
    """the operations of sequence(), plus ("shared", bow) / ("score", bow, slots) / ("fields",), as the oracle's input"""
    lines = [f"N {nwords}"]
    nslots = 0
    for op in ops:
        if op[0] == "add":
            lines.append("A " + bow_text(op[1]))
            if len(op) > 2:
                lines.append(f"G {nslots} {len(op[2])} " + " ".join(map(str, op[2])))
            nslots += 1
        elif op[0] == "erase":
            lines.append(f"E {op[1]}")
        elif op[0] == "clear":
            lines.append("C"); nslots = 0
        elif op[0] == "loop":
            lines.append(f"L {op[2]} {float(np.float32(op[4])).hex()} {len(op[3])} " + " ".join(map(str, op[3])) + " " + bow_text(op[1]))
        elif op[0] == "reloc":
            lines.append(f"R {op[2]} " + bow_text(op[1]))
        elif op[0] == "shared":
            lines.append("Q " + bow_text(op[1]))
        elif op[0] == "score":
            lines.append(f"S {len(op[2])} " + " ".join(map(str, op[2])) + " " + bow_text(op[1]))
        elif op[0] == "fields":
            lines.append("F")
        else:
            raise ValueError(op[0])
        if dump_each_query and op[0] in ("loop", "reloc"):
            lines.append("F")
    return "\n".join(lines) + "\n"


def run_oracle(exe, text):
    """the oracle's output as a list of records: ("A", slot), ("Q", common, first, score), ("S", scores), ("L" / "R", candidates,
    sharing list), ("F", six arrays)"""
    return parse_output(subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout)


def parse_output(stdout):
    out = stdout.split("\n")
    f32 = lambda t: np.float32(float.fromhex(t))
    rec, i = [], 0
    while i < len(out):
        w = out[i].split(); i += 1
        if not w:
            continue
        if w[0] == "A":
            rec.append(("A", int(w[1])))
        elif w[0] == "Q":
            rows = [out[i + k].split() for k in range(int(w[1]))]; i += int(w[1])
            rec.append(("Q", np.array([int(r[0]) for r in rows], np.int32), np.array([int(r[1]) for r in rows], np.int32),
                        np.array([f32(r[2]) for r in rows], np.float32)))
        elif w[0] == "S":
            rec.append(("S", np.array([f32(t) for t in w[2:]], np.float32)))
        elif w[0] in ("L", "R"):
            sharing = out[i].split(); i += 1
            assert sharing[0] == "W"
            rec.append((w[0], [int(t) for t in w[2:]], [int(t) for t in sharing[2:]]))
        elif w[0] == "F":
            rows = [out[i + k].split() for k in range(int(w[1]))]; i += int(w[1])
            col = lambda j, conv, t: np.array([conv(r[j]) for r in rows], t)
            rec.append(("F", (col(0, int, np.int64), col(1, int, np.int32), col(2, f32, np.float32), col(3, int, np.int64),
                              col(4, int, np.int32), col(5, f32, np.float32))))
        else:
            raise ValueError(out[i - 1])
    return rec


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
