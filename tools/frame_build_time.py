#!/usr/bin/env python3
"""Call time of making resident frames from the extractor's device results (orbm_frame_from_extractor and its camera / batch forms):
  plain   the existing entry without undistorted coordinates, 2,000 features on 640 x 480 (README's "making the frame handle" row);
  (i)     one distorted frame at the fork's settings (1,200 features, scale 1.1, 6 levels, FAST 24 / 7; 640 x 360, sHamlyn04):
          host_path = download of the keypoints + orbm_frame_from_extractor(xy_undistorted) against cam = orbm_frame_from_extractor_cam.
          host_path is fed precomputed coordinates: its host undistortion is not counted, so the gain is a lower bound;
  (ii)    64 handles of one extracted batch: singles = 64 single camera calls against batch = one orbm_frames_from_extractor call;
          singles_plain = 64 calls of the existing entry without coordinates.
Every form destroys the handles it made inside the timed region (the pool hands the blocks to the next call).
With --parent-lib PATH (a build of the parent commit's library) the forms that exist there (plain, host_path, singles_plain) are also timed
on that build, on an extractor of its own, in the same process and the same alternation: this change touches the kernel they run.
The forms alternate in one process; a figure is the median over batches of the mean of 10 calls, with the spread (min .. max over
batches) beside it.  Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_e_amd import Distortion                              # noqa: E402
from orb_slam2_e_amd._lib import SO_PATH, _one_hip_runtime, prototypes, ptr as _p   # noqa: E402
from orb_slam2_e_amd.extractor import KP_DTYPE, _Params             # noqa: E402
from orb_slam2_e_amd.synth import synth_frame, synth_frames        # noqa: E402

HAMLYN04 = (752.737796, 765.331797, 263.657845, 245.883296, -0.332222, 0.708196, 0.003904, 0.008043, 0.0)


class Build:
    """One build of the library and an extractor of its own"""

    def __init__(self, path):
        _one_hip_runtime()
        self.L = C.CDLL(path)
        for name, (restype, argtypes) in prototypes().items():
            if hasattr(self.L, name):
                fn = getattr(self.L, name)
                fn.restype, fn.argtypes = restype, argtypes
        self.new = hasattr(self.L, "orbm_frames_from_extractor")

    def extractor(self, prm, images):
        """a handle with `images` ([B, h, w]) extracted and finished"""
        L = self.L
        h = C.c_void_p()
        p = _Params(*prm, 0)
        assert L.orbx_create(C.byref(p), C.byref(h)) == 0
        B, hh, ww = images.shape
        assert L.orbx_reserve(h, ww, hh, B) == 0
        assert L.orbx_extract_batch(h, _p(images), 0, ww, hh, ww, ww * hh, B, None) == 0
        cap = L.orbx_keypoint_capacity(h)
        self.kps = np.zeros(cap, KP_DTYPE); self.desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        assert L.orbx_download(h, 0, _p(self.kps), _p(self.desc), cap, C.byref(n)) == 0
        return h, cap, n.value

    def download(self, h, cap):
        n = C.c_int(0)
        assert self.L.orbx_download(h, 0, _p(self.kps), _p(self.desc), cap, C.byref(n)) == 0

    def single(self, h, frame, xy, bounds, cam=None):
        f = C.c_void_p()
        if cam is not None:
            rc = self.L.orbm_frame_from_extractor_cam(h, frame, C.byref(cam), None, 0, *bounds, C.byref(f))
        else:
            rc = self.L.orbm_frame_from_extractor(h, frame, _p(xy) if xy is not None else None, None, 0, *bounds, C.byref(f))
        assert rc == 0
        return f

    def batch(self, h, count, bounds, cam, out):
        assert self.L.orbm_frames_from_extractor(h, 0, count, C.byref(cam), 0, *bounds, out) == 0


def measure(forms, batches, calls):
    for _ in range(3):
        for _, fn in forms:
            fn()
    times = {name: [] for name, _ in forms}
    for _ in range(batches):
        for name, fn in forms:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            times[name].append((time.perf_counter() - t0) / calls * 1e3)
    out = {}
    for name, ts in times.items():
        out[name + "_ms"] = round(float(np.median(ts)), 4)
        out[name + "_spread_ms"] = [round(min(ts), 4), round(max(ts), 4)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    builds = [("new", Build(SO_PATH))] + ([("parent", Build(a.parent_lib))] if a.parent_lib else [])
    cam = Distortion(*HAMLYN04)

    # plain: README's row
    b480 = (0.0, 0.0, 640.0, 480.0)
    forms = []
    for tag, B in builds:
        h, cap, n = B.extractor((2000, 1.2, 8, 20, 7), synth_frame(3)[None])
        forms.append(("plain_" + tag, lambda B=B, h=h: B.L.orbm_frame_destroy(B.single(h, 0, None, b480))))
    print(json.dumps(dict(measurement="plain", features=2000, image="640x480", keypoints=n, batches=a.batches, calls_per_batch=a.calls,
                          **measure(forms, a.batches, a.calls))), flush=True)

    # (i) one distorted frame at the fork's settings
    fork = (1200, 1.1, 6, 24, 7)
    fb = (C.c_float * 4)()
    assert builds[0][1].L.orbm_image_bounds(C.byref(cam), 640, 360, fb) == 0
    bnd = [float(v) for v in fb]
    img = synth_frame(3, 640, 360)[None]
    forms = []
    for tag, B in builds:
        h, cap, n = B.extractor(fork, img)
        xy = np.ascontiguousarray(np.stack([B.kps["x"][:n], B.kps["y"][:n]], 1), np.float32)
        if B.new:
            xy_un = np.zeros_like(xy)
            assert B.L.orbm_undistort_points(C.byref(cam), _p(xy), n, _p(xy_un)) == 0
            shared_xy = xy_un

            def cam_form(B=B, h=h):
                B.L.orbm_frame_destroy(B.single(h, 0, None, bnd, cam))
            forms.append(("cam_" + tag, cam_form))

        def host_path(B=B, h=h, cap=cap):
            B.download(h, cap)
            B.L.orbm_frame_destroy(B.single(h, 0, shared_xy, bnd))
        forms.append(("host_path_" + tag, host_path))
    res = measure(forms, a.batches, a.calls)
    print(json.dumps(dict(measurement="one_distorted_frame", settings=fork, image="640x360", keypoints=n, batches=a.batches,
                          calls_per_batch=a.calls, **res)), flush=True)

    # (ii) 64 handles of one batch
    imgs = synth_frames(64, 640, 360)
    forms = []
    for tag, B in builds:
        h, cap, n = B.extractor(fork, imgs)

        def singles_plain(B=B, h=h):                 # the existing entry, no coordinates: the same call on both builds
            fs = [B.single(h, f, None, bnd) for f in range(64)]
            for f in fs:
                B.L.orbm_frame_destroy(f)
        forms.append(("singles_plain_" + tag, singles_plain))
        if B.new:
            def singles(B=B, h=h):
                fs = [B.single(h, f, None, bnd, cam) for f in range(64)]
                for f in fs:
                    B.L.orbm_frame_destroy(f)
            forms.append(("singles_" + tag, singles))

            out = (C.c_void_p * 64)()

            def batch(B=B, h=h, out=out):
                B.batch(h, 64, bnd, cam, out)
                for f in out:
                    B.L.orbm_frame_destroy(f)
            forms.append(("batch_" + tag, batch))
    res = measure(forms, a.batches, a.calls)
    print(json.dumps(dict(measurement="64_handles", settings=fork, image="640x360", batches=a.batches, calls_per_batch=a.calls,
                          **res)), flush=True)


if __name__ == "__main__":
    main()
