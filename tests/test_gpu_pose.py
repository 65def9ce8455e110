"""Optimizer::PoseOptimization on the device (orbm_pose.hip) against the CPU restatement (tests/pose_only_oracle.c): exact
discrete outputs (outlier flags, ngood, rounds, iterations and trials per round), the double pose to 1e-9, the float pose to
2 ulp; the resident-frame, batch and repeated forms bit for bit; and an end-to-end step from SearchByProjection(Cur, Last).

Every scene first checks, on the restatement's side, that no discrete decision lies near its threshold: a classification
chi2 within 1e-6 (relative) of 5.991 / 7.815, an accept / reject rho within 1e-9 of 0 (exactly 0 included: once a scene has converged to the
last bits, the trials that follow decide on rounding noise -- three monocular edges, six residuals for six unknowns, always
do), Raul's stop criterion within 1e-9.  Device sin / cos / pow need not match glibc's last bit; these margins keep such a difference from flipping a
decision."""
import numpy as np
import pytest

import pose_only_oracle as po
import pose_only_scene as ps
from orb_slam2_e_amd import pose_optimization, pose_optimization_batch
from orb_slam2_e_amd.matcher import Frame, ORBmatcher, Points, View
from orb_slam2_e_amd.synth import synth_tracking_scene
from orb_slam2_e_amd.extractor import KP_DTYPE

pytestmark = pytest.mark.gpu


def _dev(p, frame=None):
    return pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"], p["Tcw"],
                             frame=frame)


def _margins_ok(st):
    assert st.min_class > 1e-6, f"a classification lies within {st.min_class:.2e} of its threshold"
    assert st.min_rho > 1e-9, st.min_rho
    assert st.min_stop > 1e-9 or st.min_stop == np.inf, st.min_stop


def _ulp_diff(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def _agree(p, got, ref):
    ng, T, out, st = got
    rng_, rT, rout, rst = ref
    hm = p["has_mp"] > 0
    assert ng == rng_
    assert np.array_equal(out[hm], rout[hm])
    assert st.rounds == rst.rounds and st.ninitial == rst.ninitial
    assert list(st.iterations) == list(rst.iterations) and list(st.trials) == list(rst.trials)
    q, rq = np.array(st.q), np.array(rst.q)
    t, rt = np.array(st.t), np.array(rst.t)
    assert np.all(np.abs(q - rq) <= 1e-9 * np.maximum(1, np.abs(rq))), (q, rq)
    assert np.all(np.abs(t - rt) <= 1e-9 * np.maximum(1, np.abs(rt))), (t, rt)
    assert _ulp_diff(T, rT).max() <= 2


CASES = {
    # name: (seed, n keypoints, stereo fraction, outlier fraction, extra make_problem arguments)
    "mono_50": (110, 60, 0.0, 0.1, {"noise_px": 2.0}),
    "stereo_50": (39, 60, 1.0, 0.1, {}),
    "mixed_500": (3, 590, 0.4, 0.2, {}),
    "mixed_2000": (4, 2350, 0.5, 0.3, {}),
    "mixed_8192": (5, 8192, 0.5, 0.25, {"fill": 1.0}),
    "stereo_3": (6, 3, 1.0, 0.0, {"fill": 1.0}),
    "mono_9": (0, 9, 0.0, 0.0, {"fill": 1.0, "noise_px": 2.0}),
    "stereo_10": (8, 10, 1.0, 0.0, {"fill": 1.0}),
    "mixed_11": (9, 11, 0.5, 0.0, {"fill": 1.0}),
    "outliers_50pct": (84, 400, 0.3, 0.5, {}),
    "clean_500": (11, 500, 0.3, 0.0, {"fill": 1.0}),
    "z0_and_behind": (12, 300, 0.3, 0.1, {"z0": 2, "behind": 5}),
    "far_start": (50, 300, 0.2, 0.1, {"rot_deg": 40.0, "trans_m": 1.5}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_restatement(name):
    seed, n, sf, of, kw = CASES[name]
    p = ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=of, **kw)
    ref = po.run(p)
    _margins_ok(ref[3])
    got = _dev(p)
    _agree(p, got, ref)
    if name == "far_start":
        assert max(ref[3].trials[i] - ref[3].iterations[i] for i in range(4)) > 0      # trials were rejected
    if name == "mono_9":
        assert ref[3].rounds == 1


def test_fewer_than_three_and_empty():
    p = ps.make_problem(20, 40, fill=0.0)
    p["has_mp"][[3, 17]] = 1
    ng, T, out, st = _dev(p)
    assert ng == 0 and st.rounds == 0 and st.ninitial == 2
    assert np.array_equal(T, p["Tcw"]) and out[3] == 0 and out[17] == 0
    p = ps.make_problem(21, 0)
    ng, T, out, st = _dev(p)
    assert ng == 0 and np.array_equal(T, p["Tcw"])


def test_resident_frame_equals_host_arrays():
    for seed, sf in ((30, 0.0), (31, 0.6)):
        p = ps.make_problem(seed, 1500, stereo_frac=sf, outlier_frac=0.2)
        k = np.zeros(len(p["octave"]), KP_DTYPE)
        k["x"], k["y"], k["octave"] = p["kp_xy"][:, 0], p["kp_xy"][:, 1], p["octave"]
        desc = np.zeros((len(k), 32), np.uint8)
        fr = Frame(k, desc, (-1e4, -1e4, 1e4, 1e4), p["uright"] if sf > 0 else None)
        host = _dev(dict(p, uright=p["uright"] if sf > 0 else None))
        res = _dev(p, frame=fr)
        fr.close()
        assert host[0] == res[0] and np.array_equal(host[1].view(np.uint32), res[1].view(np.uint32))
        assert np.array_equal(host[2], res[2]) and bytes(host[3]) == bytes(res[3])


def test_batch_equals_single_calls_and_repeats():
    rng = np.random.default_rng(40)
    probs = []
    for b in range(64):
        n = int(rng.choice([5, 9, 12, 60, 300, 700, 1500]))
        probs.append(ps.make_problem(100 + b, n, stereo_frac=float(rng.uniform(0, 1)), outlier_frac=float(rng.uniform(0, 0.4))))
    batch = pose_optimization_batch(probs, ps.CAM, ps.inv_level_sigma2())
    again = pose_optimization_batch(probs[::-1], ps.CAM, ps.inv_level_sigma2())[::-1]
    for p, b, a in zip(probs, batch, again):
        s = _dev(p)
        hm = p["has_mp"] > 0
        for x in (b, a):
            assert x[0] == s[0] and np.array_equal(x[1].view(np.uint32), s[1].view(np.uint32))
            assert np.array_equal(x[2][hm], s[2][hm]) and bytes(x[3]) == bytes(s[3])
    p = probs[7]
    r1, r2 = _dev(p), _dev(p)
    assert bytes(r1[3]) == bytes(r2[3]) and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])


@pytest.mark.parametrize("stereo", [False, True])
def test_end_to_end_after_search_by_projection_last(stereo):
    """TrackWithMotionModel's data plane: SearchByProjection(Cur, Last) from the last pose, then PoseOptimization from it."""
    # scene seeds whose restatement passes the margins: on this near noise-free scene most monocular seeds run trials whose rho
    # sits at the rounding floor once converged
    s = synth_tracking_scene(13 if stereo else 115, stereo=stereo, motion="none")
    lm = s["last_mp"]
    m = ORBmatcher(0.9, True)
    cur = Frame(s["kps"], s["desc"], s["bounds"], s["uright"])
    last = Points(s["last_valid"], s["pos"][lm], s["mp_desc"][lm], takes=s["last_takes"], octave=s["last_octave"], angle=s["last_angle"])
    view = View(*s["cam"], s["mb"], s["mbf"], s["log_scale_factor"], s["scale_factors"])
    match_kp, _, nm = m.SearchByProjectionLast(cur, view, s["Tlw"], s["Tlw"], last, s["occupied"], 15.0, not stereo)
    assert nm > 100
    has = (match_kp >= 0).astype(np.uint8)
    mp = np.zeros((len(has), 3), np.float32)
    mp[has > 0] = s["pos"][lm[match_kp[has > 0]]]
    cam = (*s["cam"], s["mbf"])
    inv = (1.0 / s["scale_factors"].astype(np.float32) ** 2).astype(np.float32)
    p = {"kp_xy": np.stack([s["kps"]["x"], s["kps"]["y"]], 1), "octave": s["kps"]["octave"],
         "uright": s["uright"] if stereo else None, "has_mp": has, "mp_pos": mp, "cam": np.array(cam, np.float32), "inv_sigma2": inv,
         "Tcw": s["Tlw"]}
    ref = po.run(p)
    _margins_ok(ref[3])
    got = _dev(p)
    res = _dev(p, frame=cur)
    cur.close()
    _agree(p, got, ref)
    assert res[0] == got[0] and np.array_equal(res[1].view(np.uint32), got[1].view(np.uint32))
    T = got[1].astype(np.float64)
    Ttrue = np.asarray(s["Tcw"], np.float64)
    assert np.abs(T[:3, :3] - Ttrue[:3, :3]).max() < 2e-3 and np.abs(T[:3, 3] - Ttrue[:3, 3]).max() < 2e-2
    assert got[0] > 0.5 * nm
