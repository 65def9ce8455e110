"""Latency of bench.py's search legs (same scenes, same calls) without the rest of the benchmark: the legs alternate batch by batch,
per call = median of the means of 30 10-call batches, with the inter-quartile range of the batch means.  To compare two builds run
it from each tree in turn, several rounds, in one session.  Prints one JSON line.
usage: python tools/search_time.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from orb_slam2_e_amd import Frame, ORBmatcher, Points, View
from orb_slam2_e_amd.synth import synth_initialization_case, synth_projection_case, synth_tracking_scene
q, qd, qa, takes, kps, desc, bounds, occ, ur = synth_projection_case(0, n=2000, nq=2000, hot=2000)
m = ORBmatcher(0.6, True); mi = ORBmatcher(0.9, True)
ik1, id1, ik2, id2, iprev, ibounds = synth_initialization_case(0)
fr = Frame(kps, desc, bounds, ur)
sc = synth_tracking_scene(11); lm = sc["last_mp"]
cur = Frame(sc["kps"], sc["desc"], sc["bounds"])
view = View(*sc["cam"], sc["mb"], sc["mbf"], sc["log_scale_factor"], sc["scale_factors"])
last = Points(sc["last_valid"], sc["pos"][lm], sc["mp_desc"][lm], takes=sc["last_takes"], octave=sc["last_octave"], angle=sc["last_angle"])
npnt = len(sc["pos"])
pts = Points(np.ones(npnt, np.uint8), sc["pos"], sc["mp_desc"], normal=sc["normal"], min_distance=sc["mind"], max_distance=sc["maxd"], takes=np.ones(npnt, np.uint8))
legs = (("search_for_initialization_2000x2200_ms", lambda: mi.SearchForInitialization(ik1, id1, ik2, id2, iprev, ibounds, 100)),
        ("search_by_projection_2000x2000_ms", lambda: m.frame_search_projection(fr, q, qd, qa, takes, occ, 95)),
        ("search_by_projection_2000x2000_host_arrays_ms", lambda: m.search_projection(q, qd, qa, takes, kps, desc, bounds, occ, ur, 95)),
        ("search_by_projection_last_frame_whole_2000x2000_ms", lambda: m.SearchByProjectionLast(cur, view, sc["Tcw"], sc["Tlw"], last, sc["occupied"], 7.0, True)),
        ("search_local_points_whole_2500x2000_ms", lambda: m.SearchByProjectionPoints(cur, view, sc["Tcw"], pts, sc["occupied"], 1.0)))
out = {}
for _, f in legs:
    for _ in range(20): f()
means = {k: [] for k, _ in legs}
for _ in range(30):                      # legs alternate batch by batch
    for k, f in legs:
        t0 = time.perf_counter()
        for _ in range(10): f()
        means[k].append((time.perf_counter() - t0) / 10 * 1e3)
for k, v in means.items():
    v = np.sort(v); out[k] = round(float(np.median(v)), 5); out[k[:-3] + "_iqr_ms"] = round(float(v[22] - v[7]), 5)
print(json.dumps(out))
