"""The glue of Tracking::TrackWithMotionModel (src/Tracking.cc:1232-1284, behind UpdateLastFrame) and Tracking::TrackLocalMap
(:1294-1320, behind UpdateLocalMap) restated in Python around the CPU oracles: oracle.search_by_projection_last /
oracle.project_points + oracle.search_projection_seq for the searches, tests/pose_only_oracle.c for PoseOptimization.  Independent of
the device; test infrastructure, never part of the product.

A frame is a dict (kps, desc, uright or None, bounds), a view a dict (cam = (fx, fy, cx, cy), mb, mbf, scale_factors,
log_scale_factor) -- a synth_tracking_scene dict serves as both -- and the pose camera is (cam5 = (fx, fy, cx, cy, mbf),
inv_sigma2).  `search` / `solve` may be replaced (the CPU tests stub them to hold the glue to known answers)."""
import numpy as np

import oracle
import pose_only_oracle as po

TH_HIGH = 95


def pose_camera(s):
    """(cam5, mvInvLevelSigma2) of a synth_tracking_scene"""
    inv = (1.0 / s["scale_factors"].astype(np.float32) ** 2).astype(np.float32)
    return np.array((*s["cam"], s["mbf"]), np.float32), inv


def search_last(fr, Tcw, Tlw, last, th, mono, check_orientation=True):
    """SearchByProjection(Cur, Last, th, mono) with every slot free -> (match_kp, match_q, nmatches)"""
    r = oracle.search_by_projection_last(fr["kps"], fr["desc"], fr["uright"], None, fr["bounds"], fr["cam"], fr["mb"], fr["mbf"], Tcw,
                                         fr["scale_factors"], Tlw, last["valid"], last["pos"], last["desc"], last["takes"], last["octave"],
                                         last["angle"], th, mono, TH_HIGH, check_orientation)
    return r[0], r[1], r[2]


def search_points(fr, Tcw, pts, occupied, th, nnratio, cos_limit=0.5):
    """Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th) -> (match_kp, match_q, nmatches, projected)"""
    T = np.asarray(Tcw, np.float32)
    npnt = len(pts["valid"])
    proj, q = oracle.project_points(0, pts["pos"], pts["normal"], pts["mind"], pts["maxd"], T[:3, :3], T[:3, 3], oracle.camera_centre(T),
                                    fr["cam"], fr["bounds"], fr["mbf"], cos_limit, fr["log_scale_factor"], fr["scale_factors"], th)
    q = q.copy(); q["r"][pts["valid"] == 0] = -1.0
    proj = proj.copy(); proj[pts["valid"] == 0] = np.zeros(1, proj.dtype); proj["level"][pts["valid"] == 0] = -1
    mk, mq, nm = oracle.search_projection_seq(q, pts["desc"], np.zeros(npnt, np.float32), pts["takes"], fr["kps"], fr["desc"], fr["bounds"],
                                              occupied, fr["uright"], TH_HIGH, nnratio, True, False)
    return mk, mq, nm, proj


def problem(fr, posecam, has, pos, Tcw):
    """the pose_only_oracle problem dict of a frame whose slot j holds a point at pos[j] where has[j]"""
    cam5, inv = posecam
    return {"kp_xy": np.stack([fr["kps"]["x"], fr["kps"]["y"]], 1), "octave": fr["kps"]["octave"], "uright": fr["uright"],
            "has_mp": np.asarray(has, np.uint8), "mp_pos": np.asarray(pos, np.float32), "cam": cam5, "inv_sigma2": inv,
            "Tcw": np.asarray(Tcw, np.float32)}


def solve_pose(fr, posecam, has, pos, Tcw):
    """Optimizer::PoseOptimization -> (ngood, Tcw_out, outlier, Stats)"""
    return po.run(problem(fr, posecam, has, pos, Tcw))


def counts(has, outlier, takes):
    """The loops behind the solve: (slots that hold a point and are not outliers, those of them whose point has Observations() > 0)
    = (nmatches, nmatchesMap) of :1257-1276 = (mnMatchesInliers with mbOnlyTracking, without) of :1301-1320."""
    ok = (np.asarray(has) > 0) & (np.asarray(outlier) == 0)
    return int(ok.sum()), int((ok & (np.asarray(takes) > 0)).sum())


def gather(match_kp, pts_pos, pts_takes):
    """keypoint j holds pts[match_kp[j]] iff match_kp[j] >= 0 -> (has, pos, takes) by keypoint index"""
    has = match_kp >= 0
    pos = np.zeros((len(match_kp), 3), np.float32); takes = np.zeros(len(match_kp), np.uint8)
    pos[has] = np.asarray(pts_pos, np.float32)[match_kp[has]]
    takes[has] = np.asarray(pts_takes, np.uint8)[match_kp[has]]
    return has.astype(np.uint8), pos, takes


def union(match_kp, pts_pos, pts_takes, base_has, base_pos, base_takes):
    """mvpMapPoints after SearchLocalPoints: a new match overwrites its slot (the search only takes a slot that holds no observed
    point, ORBmatcher.cc:87-89), every other slot keeps what the frame held -> (has, pos, takes)"""
    has, pos, takes = gather(match_kp, pts_pos, pts_takes)
    keep = (has == 0) & (np.asarray(base_has) > 0)
    pos[keep] = np.asarray(base_pos, np.float32)[keep]
    takes[keep] = np.asarray(base_takes, np.uint8)[keep]
    return (has | keep).astype(np.uint8), pos, takes


def track_with_motion_model(fr, posecam, Tcw, Tlw, last, th, mono, min_matches=20, check_orientation=True, search=search_last,
                            solve=solve_pose):
    """Tracking.cc:1232-1284.  Returns a dict: tracked, search_used, nsearch, match_kp, match_q, and -- if tracked -- has, outlier,
    Tcw_out, ngood, nmatches, nmatches_map, stats (the restatement's Stats with its margins); not tracked: Tcw_out = Tcw."""
    used = 1
    mk, mq, nm = search(fr, Tcw, Tlw, last, th, mono, check_orientation)                      # :1242
    if nm < min_matches:                                                                      # :1245-1249
        used = 2
        mk, mq, nm = search(fr, Tcw, Tlw, last, 2 * th, mono, check_orientation)
    r = dict(tracked=False, search_used=used, nsearch=nm, match_kp=mk, match_q=mq, Tcw_out=np.array(Tcw, np.float32).reshape(4, 4),
             ngood=0, nmatches=0, nmatches_map=0, outlier=None, stats=None, has=(mk >= 0).astype(np.uint8))
    if nm < min_matches:                                                                      # :1251-1252
        return r
    has, pos, takes = gather(mk, last["pos"], last["takes"])
    ng, T, out, st = solve(fr, posecam, has, pos, Tcw)                                        # :1255
    n1, n2 = counts(has, out, takes)                                                          # :1257-1276
    r.update(tracked=True, Tcw_out=T, ngood=ng, nmatches=n1, nmatches_map=n2, outlier=out, stats=st, pos=pos, takes=takes)
    return r


def track_local_map(fr, posecam, Tcw, pts, base_has, base_pos, base_takes, th, nnratio, cos_limit=0.5, search=search_points,
                    solve=solve_pose):
    """Tracking.cc:1294-1320.  Returns a dict: nsearch, match_kp, match_q, projected, has (the union), outlier, Tcw_out, ngood,
    nmatches (inliers with mbOnlyTracking), nmatches_map (mnMatchesInliers), stats."""
    occupied = ((np.asarray(base_has) > 0) & (np.asarray(base_takes) > 0)).astype(np.uint8)   # ORBmatcher.cc:87-89
    mk, mq, nm, proj = search(fr, Tcw, pts, occupied, th, nnratio, cos_limit)                 # :1294
    has, pos, takes = union(mk, pts["pos"], pts["takes"], base_has, base_pos, base_takes)
    ng, T, out, st = solve(fr, posecam, has, pos, Tcw)                                        # :1297
    n1, n2 = counts(has, out, takes)                                                          # :1301-1320
    return dict(tracked=True, search_used=1, nsearch=nm, match_kp=mk, match_q=mq, projected=proj, has=has, pos=pos, takes=takes, outlier=out,
                Tcw_out=T, ngood=ng, nmatches=n1, nmatches_map=n2, stats=st)


def last_of(s):
    """the last frame's points of a synth_tracking_scene, as search_last takes them"""
    lm = s["last_mp"]
    return dict(valid=s["last_valid"], pos=s["pos"][lm], desc=s["mp_desc"][lm], takes=s["last_takes"], octave=s["last_octave"],
                angle=s["last_angle"])


def rotate_y(T, deg):
    """the pose T with the camera turned by deg about its own y axis (a predicted pose that is off)"""
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    return (R @ np.asarray(T, np.float64)).astype(np.float32)


def margins_ok(st):
    """no discrete decision of the restatement near its threshold (tests/test_gpu_pose.py: _margins_ok)"""
    assert st.min_class > 1e-6, f"a classification lies within {st.min_class:.2e} of its threshold"
    assert st.min_rho > 1e-9, st.min_rho
    assert st.min_stop > 1e-9 or st.min_stop == np.inf, st.min_stop


def local_map_case(s, seed=1, base_frac=0.3):
    """A TrackLocalMap call on a synth_tracking_scene: the frame already holds the true point of base_frac of its keypoints (about
    70 % of them observed; half of the unobserved slots hold some other point instead, so that the search replaces them), the local
    map is every map point the frame does not hold (90 % valid, 80 % observed).
    Returns (pts dict, base_has, base_pos, base_takes)."""
    rng = np.random.default_rng(seed)
    n, npnt = len(s["kps"]), len(s["pos"])
    bh = ((rng.random(n) < base_frac) & (s["src"] >= 0)).astype(np.uint8)
    bpos = np.zeros((n, 3), np.float32); bpos[bh > 0] = s["pos"][s["src"][bh > 0]]
    bt = ((rng.random(n) < 0.7) & (bh > 0)).astype(np.uint8)
    stale = (bh > 0) & (bt == 0) & (rng.random(n) < 0.5)     # an unobserved slot that holds another point: its own is still in the map
    bpos[stale] = s["pos"][rng.integers(0, npnt, int(stale.sum()))]
    valid = (rng.random(npnt) < 0.9).astype(np.uint8); valid[s["src"][(bh > 0) & ~stale]] = 0
    takes = (rng.random(npnt) < 0.8).astype(np.uint8)
    pts = dict(valid=valid, pos=s["pos"], normal=s["normal"], mind=s["mind"], maxd=s["maxd"], desc=s["mp_desc"], takes=takes)
    return pts, bh, bpos, bt


def base_from_motion_model(s, mk, outlier, last):
    """mvpMapPoints after TrackWithMotionModel's discard loop, as TrackLocalMap's base, and the local map around it"""
    bh = ((mk >= 0) & (np.asarray(outlier) == 0)).astype(np.uint8)
    _, bpos, bt = gather(np.where(bh > 0, mk, -1).astype(np.int32), last["pos"], last["takes"])
    npnt = len(s["pos"])
    valid = np.ones(npnt, np.uint8); valid[s["last_mp"][mk[bh > 0]]] = 0
    pts = dict(valid=valid, pos=s["pos"], normal=s["normal"], mind=s["mind"], maxd=s["maxd"], desc=s["mp_desc"], takes=np.ones(npnt, np.uint8))
    return pts, bh, bpos, bt
