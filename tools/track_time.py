"""Latency of the tracking functions as ONE call (orbm_track_with_motion_model / orbm_track_local_map) against the two-call form
they replace -- the search, the host gather of has_mp / mp_pos, orbm_frame_pose_optimization -- on the 2000-keypoint tracking scene,
in one process, the two forms alternating: medians of 10-call batch means, and the two-call form's own run-to-run spread (the
inter-quartile range of its batch means) as the yardstick for "not slower".
Per-kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/track_time.py` (a run of its own).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import track_reference as tr  # noqa: E402
from orb_slam2_e_amd import pose_optimization  # noqa: E402
from orb_slam2_e_amd.matcher import Frame, ORBmatcher, Points, View  # noqa: E402
from orb_slam2_e_amd.synth import synth_tracking_scene  # noqa: E402


def _batch_means_ms(fns, batches, per_batch=10):
    """fns alternate batch by batch; returns one list of batch means (ms per call) per function"""
    out = [[] for _ in fns]
    for _ in range(batches):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(per_batch):
                fn()
            out[k].append(1e3 * (time.perf_counter() - t0) / per_batch)
    return out


def _row(one, two):
    q1, q3 = np.percentile(two, [25, 75])
    return {"one_call_ms": round(float(np.median(one)), 4), "two_calls_ms": round(float(np.median(two)), 4),
            "two_calls_iqr_ms": round(float(q3 - q1), 4), "gain_ms": round(float(np.median(two) - np.median(one)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--stereo", type=int, default=1)
    a = ap.parse_args()
    stereo = bool(a.stereo)
    s = synth_tracking_scene(13 if stereo else 107, stereo=stereo, motion="none")
    pc, last = tr.pose_camera(s), tr.last_of(s)
    view = View(*s["cam"], s["mb"], s["mbf"], s["log_scale_factor"], s["scale_factors"])
    cur = Frame(s["kps"], s["desc"], s["bounds"], s["uright"])
    lastp = Points(last["valid"], last["pos"], last["desc"], takes=last["takes"], octave=last["octave"], angle=last["angle"])
    m = ORBmatcher(0.9, True)
    th, mono, T = (7.0 if stereo else 15.0), not stereo, s["Tlw"]

    def mm_one():
        return m.TrackWithMotionModel(cur, view, *pc, T, T, lastp, th, mono)

    def mm_two():
        mk, _, _ = m.SearchByProjectionLast(cur, view, T, T, lastp, None, th, mono)
        has, pos, _ = tr.gather(mk, last["pos"], last["takes"])
        return pose_optimization(None, None, None, has, pos, pc[0], pc[1], T, frame=cur)

    pts, bh, bpos, bt = tr.local_map_case(s)
    ptsp = Points(pts["valid"], pts["pos"], pts["desc"], normal=pts["normal"], min_distance=pts["mind"], max_distance=pts["maxd"],
                  takes=pts["takes"])
    occ = ((bh > 0) & (bt > 0)).astype(np.uint8)
    m8 = ORBmatcher(0.8, True)

    def lm_one():
        return m8.TrackLocalMap(cur, view, *pc, T, ptsp, bh, bpos, bt, 1.0)

    def lm_two():
        mk = m8.SearchByProjectionPoints(cur, view, T, ptsp, occ, 1.0)[0]
        has, pos, _ = tr.union(mk, pts["pos"], pts["takes"], bh, bpos, bt)
        return pose_optimization(None, None, None, has, pos, pc[0], pc[1], T, frame=cur)

    for fn in (mm_one, mm_two, lm_one, lm_two):
        for _ in range(10):
            fn()
    mm = _batch_means_ms([mm_one, mm_two], a.batches)
    waits_mm = ORBmatcher.last_track_waits()
    lm = _batch_means_ms([lm_one, lm_two], a.batches)
    waits_lm = ORBmatcher.last_track_waits()
    cur.close()
    print(json.dumps({"keypoints": len(s["kps"]), "stereo": stereo, "motion_model": dict(_row(*mm), waits=waits_mm),
                      "local_map": dict(_row(*lm), waits=waits_lm)}))


if __name__ == "__main__":
    main()
