"""bench.py --dump-outputs: what it writes is the last timed step's result as the path's caller receives it -- equal, frame by
frame, to the CPU oracle on the same frames (bench.verify_against_oracle, the checker of a --full run), and the same from run to run.
bench.py runs as a child process, as it is run for a measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"keypoints", "descriptors", "keypoint_counts", "match_best_dist", "match_second_dist", "match_best_idx", "match12", "match_count"}


def _bench_dump(tmp_path, steps):
    d = tmp_path / f"dump_{steps}"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    return {f[:-4]: np.load(d / f) for f in os.listdir(d) if f.endswith(".npy")}


@pytest.mark.gpu
def test_bench_dump_is_the_oracles_result_and_repeats(tmp_path):
    import bench
    from orb_slam2_e_amd.extractor import KP_DTYPE
    from orb_slam2_e_amd.synth import synth_sequence

    d = _bench_dump(tmp_path, 7)         # 7 steps over the 3 pipeline contexts: the last one ran on context 0
    assert set(d) == NAMES
    assert all(a.dtype == np.float32 for a in d.values()) and sum(a.nbytes for a in d.values()) <= 64 << 20
    B = bench.BATCH
    counts = d["keypoint_counts"].astype(np.int64)
    assert counts.shape == (B,) and counts.min() > 0
    off = np.concatenate([[0], np.cumsum(counts)])
    assert all(len(d[k]) == off[-1] for k in NAMES - {"keypoint_counts", "match_count"})
    # back to the per-frame, fixed-capacity layout the checker takes (rows past counts[f] are never looked at)
    cap = int(counts.max())
    kps = np.zeros((B, cap), KP_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    best, second, idx, m12 = (np.zeros((B, cap), np.int32) for _ in range(4))
    for f in range(B):
        rows, n = slice(off[f], off[f + 1]), counts[f]
        for j, name in enumerate(KP_DTYPE.names):
            kps[name][f, :n] = d["keypoints"][rows, j].astype(KP_DTYPE[name])
        desc[f, :n] = d["descriptors"][rows].astype(np.uint8)
        for dst, key in ((best, "match_best_dist"), (second, "match_second_dist"), (idx, "match_best_idx"), (m12, "match12")):
            dst[f, :n] = d[key][rows].astype(np.int32)
    frames = synth_sequence(B, bench.W, bench.H)
    ok, why = bench.verify_against_oracle(frames, kps, desc, counts, best, second, idx, m12, d["match_count"].astype(np.int32),
                                          (np.arange(B) + 1) % B)
    assert ok, why
    d2 = _bench_dump(tmp_path, 5)        # another run whose last step ran on context 1: the same bits
    assert set(d2) == NAMES and all(np.array_equal(d[k], d2[k]) for k in NAMES)
