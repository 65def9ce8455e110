"""The table behind tests/test_gpu_workspace_contents.py and tests/test_cpu_workspace_sites.py: one case (at least) per place where
a matcher-side entry point leases a pooled workspace (orbm_detail::StagedCall / WorkspaceLease, DESIGN.md "What a call may assume
about its workspace").

A case runs ONE entry point (or the few calls that make one site reachable) on a small scene of that unit's own *_scenes.py module
and returns (the bytes of every output, the entry's host-wait count or None where it reports none).  `check` holds the baseline to
the unit's existing comparison with its oracle or restatement (with that comparison's own margins where it has any: the scenes of
those cases are the ones the unit's test module passes them on), so that a wrong answer that does not depend on the arena cannot
pass for right.  Every case has one.

SITES names every declaration of a lease in csrc/, per file, in the order of the file: test_cpu_workspace_sites.py counts the
declarations and fails when a file holds one that no case is tagged with."""
import ctypes as C
import functools

import numpy as np

SITES = {
    "orbm_match.hip": ["orbm_match_bruteforce", "orbm_match_candidates", "orbm_distinctive_descriptors", "orbm_vocab_create",
                       "orbm_bow_transform", "orbm_hamming_matrix"],
    "orbm_frame.hip": ["orbm_frame_create", "frame_from_extractor", "orbm_frames_from_extractor", "orbm_undistort_points"],
    "orbm_window.hip": ["search_window_core", "search_map_core", "search_map_poses_core", "orbm_fuse_keyframes"],
    "orbm_search.hip": ["run_sequential", "orbm_project_points", "bow_pairs_launch", "orbm_search_by_sim3"],
    "orbm_kfdb.hip": ["orbm_kfdb_add", "orbm_kfdb_erase", "orbm_kfdb_query", "orbm_kfdb_score"],
    "orbm_triang.hip": ["triang_host_arrays", "orbm_frame_search_for_triangulation", "orbm_create_new_map_points"],
    "orbm_pose.hip": ["pose_host", "orbm_frame_pose_optimization"],
    "orbm_pose_nr.hip": ["orbm_pose_optimization_nr"],
    "orbm_sim3.hip": ["orbm_sim3_hypotheses"],
    "orbm_sim3opt.hip": ["orbm_optimize_sim3"],
    "orbm_init.hip": ["orbm_init_find_models", "orbm_init_check_rt"],
    "orbm_pnp.hip": ["orbm_pnp_hypotheses"],
    # not call sites of their own: the member every StagedCall holds, and the stream-only lease of the accessors' copies
    "orbm_internal.h": ["StagedCall::lease"],
    "orbm_search_internal.h": ["copy_and_wait"],
}
NOT_A_CALL = {"orbm_internal.h/StagedCall::lease"}

# What the cases borrow from the units' own test modules (imported where a case runs, so that loading this table needs no device):
# their comparisons with the restatements and the scene builders those comparisons were tuned on.  tests/test_cpu_workspace_sites.py
# imports every name, so a rename shows on the CPU.
HELPERS = {
    "test_cpu_sim3_opt": ["M", "_ints", "_dev"],
    "test_gpu_bow": ["_synthetic_vocabulary"],
    "test_gpu_create_points": ["DeviceScene"],
    "test_gpu_init": ["check_against_restatement", "check_rt_against_restatement", "rt_scene"],
    "test_gpu_match": ["_triangulation_case"],
    "test_gpu_pnp": ["_assert_equal"],
    "test_gpu_pose": ["CASES", "_agree", "_margins_ok"],
    "test_gpu_pose_nr": ["SCENES", "Case", "_bytes", "_parity"],
    "test_gpu_sim3": ["check_against_restatement"],
    "test_gpu_sim3_opt": ["D_CPU", "_vec"],
    "test_gpu_track": ["_last", "_points", "_same_bits", "_two_calls_lm", "_two_calls_mm"],
}

BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _b(*arrays):
    """the bytes of the outputs, one entry each"""
    out = []
    for a in arrays:
        if isinstance(a, (C.Structure, bytes)):
            out.append(bytes(a))
        elif isinstance(a, (int, float, bool, np.integer, np.floating)):
            out.append(repr(a).encode())
        else:
            out.append(np.ascontiguousarray(a).tobytes())
    return out


class Case:
    def __init__(self, name, sites, run, check=None, weight=1):
        self.name, self.sites, self.run, self.check, self.weight = name, tuple(sites), run, check, weight
        for s in self.sites:
            f, fn = s.split("/")
            assert fn in SITES[f], s

    def __repr__(self):
        return self.name


CASES = []


def case(name, sites, weight=1):
    """run() -> (outputs, waits[, what check() needs]); weight: the rough size of the call's arena, for the chains"""
    def deco(make):
        run, check = make()
        CASES.append(Case(name, sites, run, check, weight))
        return make
    return deco


def _lib():
    from orb_slam2_e_amd._lib import lib
    return lib()


def _search_waits():
    return _lib().orbm_debug_last_search_waits()


class forced_sequential:
    def __enter__(self):
        self.prev = _lib().orbm_debug_force_sequential_resolver(1)

    def __exit__(self, *exc):
        _lib().orbm_debug_force_sequential_resolver(self.prev)


# ------------------------------------------------------------------------------------------------------------ orbm_match

@case("match_bruteforce", ["orbm_match.hip/orbm_match_bruteforce"])
def _():
    from orb_slam2_e_amd import ORBmatcher
    from orb_slam2_e_amd.synth import synth_descriptors

    @functools.lru_cache(None)
    def scene():
        A, B, _ = synth_descriptors(330, seed=9, n_replace=30)
        return A, B[:301]

    def run():
        return _b(*ORBmatcher(0.6).match_bruteforce(*scene())), None

    def check(out):
        import oracle
        assert out == _b(*oracle.match_bruteforce(*scene()))
    return run, check


def _cand_scene():
    from orb_slam2_e_amd.synth import synth_descriptors
    rng = np.random.default_rng(11)
    A, B, _ = synth_descriptors(260, seed=9, n_replace=30)
    off, idx = [0], []
    for _i in range(len(A)):
        idx.extend(rng.integers(0, len(B), size=int(rng.integers(0, 40))).tolist())
        off.append(len(idx))
    return A, B, off, idx


@case("match_candidates", ["orbm_match.hip/orbm_match_candidates"])
def _():
    from orb_slam2_e_amd import ORBmatcher
    scene = functools.lru_cache(None)(_cand_scene)

    def run():
        return _b(*ORBmatcher().match_candidates(*scene())), None

    def check(out):
        import oracle
        assert out == _b(*oracle.match_candidates(*scene()))
    return run, check


@case("distinctive_descriptors", ["orbm_match.hip/orbm_distinctive_descriptors"])
def _():
    from orb_slam2_e_amd import ORBmatcher

    @functools.lru_cache(None)
    def scene():
        rng = np.random.default_rng(5)
        sizes = np.concatenate([[0, 1, 2, 3, 128, 129, 130], rng.integers(1, 60, 40)])      # above 128: the row-by-row histogram path
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        base = rng.integers(0, 256, (len(sizes), 32), dtype=np.uint8)
        desc = np.concatenate([base[i] ^ np.packbits(rng.random((n, 256)) < 0.1, axis=1, bitorder="little") for i, n in enumerate(sizes) if n > 0])
        return desc, off

    def run():
        return _b(ORBmatcher.distinctive_descriptors(*scene())), None

    def check(out):
        import oracle
        assert out == _b(oracle.distinctive_descriptors(*scene()))
    return run, check


@case("vocabulary_descend", ["orbm_match.hip/orbm_vocab_create", "orbm_match.hip/orbm_bow_transform"])
def _():
    @functools.lru_cache(None)
    def scene():
        from test_gpu_bow import _synthetic_vocabulary
        off, ids, desc, word, weight, L = _synthetic_vocabulary()
        rng = np.random.default_rng(1)
        leaves = np.where(word >= 0)[0]
        feats = desc[rng.choice(leaves, 300)] ^ np.packbits(rng.random((300, 256)) < 0.04, axis=1, bitorder="little")
        return off, ids, desc, word, weight, L, feats

    def run():
        from orb_slam2_e_amd.vocabulary import ORBVocabulary
        off, ids, desc, word, weight, L, feats = scene()
        voc = ORBVocabulary(off, ids, desc, word, weight, L)       # (the upload of the tree: a lease for its stream)
        return _b(*voc.descend(feats, 4)), None

    def check(out):
        import oracle
        off, ids, desc, word, weight, L, feats = scene()
        assert out == _b(*oracle.bow_descend(off, ids, desc, word, weight, L, feats, 4))
    return run, check


@case("hamming_matrix", ["orbm_match.hip/orbm_hamming_matrix"])
def _():
    from orb_slam2_e_amd import ORBmatcher
    from orb_slam2_e_amd.synth import synth_descriptors

    @functools.lru_cache(None)
    def scene():
        A, B, _ = synth_descriptors(300, seed=3, n_replace=30)
        return A[:257], B[:211]

    def run():
        return _b(ORBmatcher.hamming_matrix(*scene())), None

    def check(out):
        import oracle
        assert out == _b(oracle.hamming_matrix(*scene()))
    return run, check


# ------------------------------------------------------------------------------------------------------------ orbm_frame

@functools.lru_cache(None)
def _window_scene(n=400, nq=300, crowd=40, seed=None):
    """the scene of tests/test_gpu_search_paths.py, smaller: a crowd of keypoints inside one window (crowd > 256: the window lists
    outgrow their 256-entry regions)"""
    from orb_slam2_e_amd import ORBmatcher
    from orb_slam2_e_amd.extractor import KP_DTYPE
    rng = np.random.default_rng(crowd if seed is None else seed)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.uniform(0, 640, n); kps["y"] = rng.uniform(0, 480, n)
    kps["x"][:crowd] = rng.uniform(300, 330, crowd); kps["y"][:crowd] = rng.uniform(200, 230, crowd)
    kps["octave"] = rng.integers(0, 3, n); kps["angle"] = rng.uniform(0, 360, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    src = rng.integers(0, n, nq); src[:nq // 3] = rng.integers(0, crowd, nq // 3)
    q = np.zeros(nq, ORBmatcher.WQ_DTYPE)
    q["u"] = kps["x"][src] + rng.normal(0, 1, nq); q["v"] = kps["y"][src] + rng.normal(0, 1, nq)
    q["r"] = 40.0; q["min_level"] = 0; q["max_level"] = 2; q["xr"] = q["u"]
    qd = desc[src] ^ np.packbits(rng.random((nq, 256)) < 0.05, axis=1, bitorder="little")
    qa = ((kps["angle"][src] + 7.0) % 360).astype(np.float32)
    return q, qd, qa, np.ones(nq, np.uint8), kps, desc, BOUNDS, np.zeros(n, np.uint8)


@case("frame_create", ["orbm_frame.hip/orbm_frame_create", "orbm_search_internal.h/copy_and_wait", "orbm_window.hip/search_window_core"])
def _():
    def run():
        """a frame made (on a recycled block, when the pool holds one), read back, searched and destroyed"""
        from orb_slam2_e_amd import Frame, ORBmatcher
        q, qd, _, _, kps, desc, bounds, occ = _window_scene()
        f = Frame(kps, desc, bounds)
        perm, cell_off = f.layout()
        found = ORBmatcher(0.8).frame_search_window(f, q, qd, occ)
        xy = f.keypoints_un()
        waits = Frame.last_build_waits()
        f.close()
        return _b(perm, cell_off, xy, *found), waits

    def check(out):
        import oracle
        q, qd, _, _, kps, desc, bounds, occ = _window_scene()
        assert out[3:] == _b(*oracle.search_window(q, qd, kps, desc, bounds, occ, None))
        assert out[2] == _b(np.stack([kps["x"], kps["y"]], 1).astype(np.float32))[0]
    return run, check


@functools.lru_cache(None)
def _extracted():
    """an extractor holding a batch of three frames (the second blank), and the camera of tests/test_gpu_frame_undistort.py"""
    import undistort_reference as ur
    from orb_slam2_e_amd import ORBextractor
    from orb_slam2_e_amd.matcher import Distortion
    from orb_slam2_e_amd.synth import synth_frame
    ex = ORBextractor(500, 1.2, 8, 20, 7)
    ex.extract_batch(np.stack([synth_frame(0), np.full((480, 640), 128, np.uint8), synth_frame(2)]))
    return ex, Distortion(*ur.CAMERAS["sHamlyn04"][0])


def _frame_bytes(f):
    perm, cell_off = f.layout()
    return _b(np.int32(f.n), np.int32(f.ns), perm, cell_off, f.keypoints_un())


@case("frame_from_extractor", ["orbm_frame.hip/frame_from_extractor", "orbm_search_internal.h/copy_and_wait"])
def _():
    NARROW = (40.0, 30.0, 600.0, 450.0)

    def run():
        from orb_slam2_e_amd import Frame
        ex, cam = _extracted()
        f = Frame.from_extractor(ex, 2, NARROW, camera=cam)
        waits = Frame.last_build_waits()
        out = _frame_bytes(f)
        f.close()
        return out, waits

    def check(out):
        """the camera form against the host undistortion form (tests/test_gpu_frame_undistort.py's equality)"""
        from orb_slam2_e_amd import Frame
        from orb_slam2_e_amd.matcher import undistort_points
        ex, cam = _extracted()
        plain = Frame.from_extractor(ex, 2, NARROW)
        xy = plain.keypoints_un(); plain.close()
        g = Frame.from_extractor(ex, 2, NARROW, xy_undistorted=undistort_points(cam, xy))
        ref = _frame_bytes(g); g.close()
        assert out == ref and len(xy) > 300
    return run, check


@case("frames_from_extractor", ["orbm_frame.hip/orbm_frames_from_extractor"], weight=2)
def _():
    NARROW = (40.0, 30.0, 600.0, 450.0)

    def run():
        from orb_slam2_e_amd import Frame
        ex, cam = _extracted()
        frames = Frame.batch_from_extractor(ex, 0, 3, NARROW, camera=cam)
        waits = Frame.last_build_waits()
        out = [b for f in frames for b in _frame_bytes(f)]
        for f in frames:
            f.close()
        return out, waits

    def check(out):
        from orb_slam2_e_amd import Frame
        ex, cam = _extracted()
        ref = []
        for k in range(3):
            f = Frame.from_extractor(ex, k, NARROW, camera=cam)
            ref += _frame_bytes(f); f.close()
        assert out == ref
    return run, check


@case("undistort_points", ["orbm_frame.hip/orbm_undistort_points"])
def _():
    @functools.lru_cache(None)
    def scene():
        import undistort_reference as ur
        rng = np.random.default_rng(3)
        return ur.CAMERAS["sHamlyn04"][0], np.stack([rng.uniform(0, 640, 333), rng.uniform(0, 480, 333)], 1).astype(np.float32)

    def run():
        from orb_slam2_e_amd.matcher import Distortion, undistort_points
        cam, pts = scene()
        got = undistort_points(Distortion(*cam), pts)
        return _b(got), None, got

    def check(out, got):
        import undistort_reference as ur
        cam, pts = scene()
        assert ur.same_bits_or_both_not_finite(got, ur.undistort(cam, pts)) and np.isfinite(got).all()
    return run, check


# ----------------------------------------------------------------------------------------------------------- orbm_window

@case("search_window_and_fuse", ["orbm_window.hip/search_window_core"])
def _():
    SG = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)

    def run():
        from orb_slam2_e_amd import ORBmatcher
        q, qd, _, _, kps, desc, bounds, occ = _window_scene()
        m = ORBmatcher(0.8)
        return _b(*m.search_window(q, qd, kps, desc, bounds, occ, None), *m.search_fuse(q, qd, kps, desc, bounds, None, SG)), None

    def check(out):
        import oracle
        q, qd, _, _, kps, desc, bounds, occ = _window_scene()
        assert out == _b(*oracle.search_window(q, qd, kps, desc, bounds, occ, None), *oracle.search_fuse(q, qd, kps, desc, bounds, None, SG))
    return run, check


_MAP_ONE, _MAP_POSES = (4, 64, 100, 2, 15.0), (2, 130, 300, 3, 3.0)       # tests/map_poses_scenes.py: the two smallest


@functools.lru_cache(None)
def _map_handles(sc):
    import map_poses_scenes as mp
    from orb_slam2_e_amd import Frame, MapSnapshot
    s = mp.scene(*sc)
    return s, Frame(s["kps"], s["desc"], BOUNDS), MapSnapshot(s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"])


@case("search_by_projection_map", ["orbm_window.hip/search_map_core"])
def _():
    def run():
        from orb_slam2_e_amd import ORBmatcher
        s, F, _ = _map_handles(_MAP_ONE)
        one = ORBmatcher(0.6).frame_search_by_projection_map(F, s["has_mp"], s["pos"], s["nrm"], s["mind"], s["maxd"], s["mp_desc"], s["Rcw"][0],
                                                             s["tcw"][0], s["cam"], s["sf"], s["th"])
        return _b(*one), None

    def check(out):
        import map_poses_scenes as mp
        assert out == _b(*mp.oracle_pose(mp.scene(*_MAP_ONE), 0))
    return run, check


@case("map_poses", ["orbm_window.hip/search_map_poses_core"], weight=2)
def _():
    def run():
        from orb_slam2_e_amd import ORBmatcher
        s, F, snap = _map_handles(_MAP_POSES)
        got = ORBmatcher(0.6).frame_search_by_projection_map_poses(F, s["has_mp"], snap, s["Rcw"], s["tcw"], s["cam"], s["sf"], s["th"], True)
        return _b(*got), ORBmatcher.last_map_poses_waits()

    def check(out):
        import map_poses_scenes as mp
        assert out == _b(*mp.oracle_rows(*_MAP_POSES))
    return run, check


@functools.lru_cache(None)
def _fuse_scene():
    import fuse_keyframes_scenes as S
    return S.random_scene(11, K=3, U=120, nclutter=60, ndup=16)


@case("fuse_keyframes", ["orbm_window.hip/orbm_fuse_keyframes"], weight=2)
def _():
    def run():
        import fuse_keyframes_scenes as S
        from orb_slam2_e_amd import ORBmatcher
        sc = _fuse_scene()
        best, idx, proj = ORBmatcher(0.8).fuse_keyframes_rows([t.device() for t in sc.targets], sc.pos, sc.nrm, sc.mind, sc.maxd, sc.list_descriptors(),
                                                              S.LOGSF, S.SF, S.INV_SIGMA2, sc.th, None, False, True)
        return _b(best, idx, proj), ORBmatcher.last_fuse_keyframes_rows_waits()

    def check(out):
        import fuse_keyframes_reference as R
        import fuse_keyframes_scenes as S
        from orb_slam2_e_amd import ORBmatcher
        sc = _fuse_scene()
        rb, ri, rv = R.candidate_rows(sc, sc.targets, np.arange(len(sc.lst)), sc.list_descriptors(), None, False)
        proj = np.frombuffer(out[2], ORBmatcher.PROJ_DTYPE).reshape(len(sc.targets), -1)
        assert out[:2] == _b(rb, ri) and np.array_equal(proj["visible"], rv) and (rb < 256).sum() > 30
    return run, check


# ----------------------------------------------------------------------------------------------------------- orbm_search

def _projection_case(name, scene, sequential=False):
    """orbm_search_projection on a window scene: run_sequential with the caller's windows"""
    @case(name, ["orbm_search.hip/run_sequential"])
    def _():
        def run():
            from orb_slam2_e_amd import ORBmatcher
            q, qd, qa, takes, kps, desc, bounds, occ = scene()
            m = ORBmatcher(0.8, True)
            if sequential:
                with forced_sequential():
                    got = m.search_projection(q, qd, qa, takes, kps, desc, bounds, occ, None, 95)
            else:
                got = m.search_projection(q, qd, qa, takes, kps, desc, bounds, occ, None, 95)
            return _b(*got), _search_waits()

        def check(out):
            import oracle
            q, qd, qa, takes, kps, desc, bounds, occ = scene()
            ref = oracle.search_projection_seq(q, qd, qa, takes, kps, desc, bounds, occ, None, 95, 0.8, False, True)
            assert out == _b(*ref) and ref[2] > 50
        return run, check


# a list overflows when a window holds more than 256 keypoints of the levels it asks for: 40 never do, 420 in a 30 x 30 px crowd do
_projection_case("projection_windows", lambda: _window_scene(400, 300, 40))
_projection_case("projection_windows_overflow", lambda: _window_scene(700, 300, 420))
_projection_case("projection_windows_sequential", lambda: _window_scene(400, 300, 40), sequential=True)
_projection_case("projection_windows_overflow_sequential", lambda: _window_scene(700, 300, 420), sequential=True)
# waits a case reports on the common path of its route (the named defect: a stale word must not add to them)
EXPECTED_WAITS = {"projection_windows": 1, "projection_windows_sequential": 1, "projection_windows_overflow": 3,
                  "projection_windows_overflow_sequential": 3, "track_motion_model": 1, "track_local_map": 1}


@functools.lru_cache(None)
def _bow_scene():
    from orb_slam2_e_amd.synth import synth_bow_case
    from orb_slam2_e_amd.vocabulary import feature_vector_arrays
    d1, a1, node1, keep1, valid1, d2, a2, node2, keep2, valid2 = synth_bow_case(0, 300, 320, 12)
    return feature_vector_arrays(node1, keep1), valid1, d1, a1, feature_vector_arrays(node2, keep2), valid2, d2, a2


def _bow_case(name, sequential):
    @case(name, ["orbm_search.hip/run_sequential"])
    def _():
        def run():
            from orb_slam2_e_amd import ORBmatcher
            m = ORBmatcher(0.7, True)
            if sequential:                  # one workgroup per vocabulary node: the segments
                with forced_sequential():
                    got = m.SearchByBoW(*_bow_scene(), True)
            else:
                got = m.SearchByBoW(*_bow_scene(), True)
            return _b(*got), _search_waits()

        def check(out):
            import oracle
            fv1, v1, d1, a1, fv2, v2, d2, a2 = _bow_scene()
            ref = oracle.search_by_bow(fv1, v1, d1, a1, fv2, v2, d2, a2, True, 0.7, True)
            assert out == _b(*ref) and ref[2] > 40
        return run, check


_bow_case("search_by_bow", False)
_bow_case("search_by_bow_sequential", True)


@functools.lru_cache(None)
def _init_search_scene():
    from orb_slam2_e_amd.synth import synth_initialization_case
    return synth_initialization_case(1, 300, 330)


def _init_search_case(name, sequential):
    @case(name, ["orbm_search.hip/run_sequential"])
    def _():
        def run():
            from orb_slam2_e_amd import ORBmatcher
            k1, d1, k2, d2, prev, bounds = _init_search_scene()
            m = ORBmatcher(0.9, True)
            if sequential:
                with forced_sequential():
                    got = m.SearchForInitialization(k1, d1, k2, d2, prev, bounds, 100)
            else:
                got = m.SearchForInitialization(k1, d1, k2, d2, prev, bounds, 100)
            return _b(*got), _search_waits()

        def check(out):
            import oracle
            k1, d1, k2, d2, prev, bounds = _init_search_scene()
            assert out == _b(*oracle.search_for_initialization(k1, d1, k2, d2, prev, bounds, 100, 0.9, True))
        return run, check


_init_search_case("search_for_initialization", False)
_init_search_case("search_for_initialization_sequential", True)


@functools.lru_cache(None)
def _tracking(seed, stereo=False, motion="none"):
    from orb_slam2_e_amd.synth import synth_tracking_scene
    return synth_tracking_scene(seed, n=700, nmp=900, stereo=stereo, motion=motion)


@functools.lru_cache(None)
def _tracking_frame(seed, stereo=False, motion="none", second=False):
    from orb_slam2_e_amd import Frame
    s = _tracking(seed, stereo, motion)
    return Frame(s["kps2"], s["desc2"], s["bounds"]) if second else Frame(s["kps"], s["desc"], s["bounds"], s["uright"])


def _view(s):
    from orb_slam2_e_amd import View
    return View(*s["cam"], s["mb"], s["mbf"], s["log_scale_factor"], s["scale_factors"])


@case("search_by_projection_last", ["orbm_search.hip/run_sequential"], weight=2)
def _():
    def run():
        """a whole-function form: the projection prefix uploads the staged block inside its own launch"""
        from orb_slam2_e_amd import ORBmatcher, Points
        s = _tracking(13, True, "forward"); lm = s["last_mp"]
        last = Points(s["last_valid"], s["pos"][lm], s["mp_desc"][lm], takes=s["last_takes"], octave=s["last_octave"], angle=s["last_angle"])
        got = ORBmatcher(0.9, True).SearchByProjectionLast(_tracking_frame(13, True, "forward"), _view(s), s["Tcw"], s["Tlw"], last, s["occupied"], 7.0,
                                                           False, want_queries=True)
        return _b(*got), _search_waits()

    def check(out):
        import oracle
        s = _tracking(13, True, "forward"); lm = s["last_mp"]
        ref = oracle.search_by_projection_last(s["kps"], s["desc"], s["uright"], s["occupied"], s["bounds"], s["cam"], s["mb"], s["mbf"],
                                               s["Tcw"], s["scale_factors"], s["Tlw"], s["last_valid"], s["pos"][lm], s["mp_desc"][lm],
                                               s["last_takes"], s["last_octave"], s["last_angle"], 7.0, False)
        assert out[:3] == _b(*ref[:3]) and ref[2] > 30
    return run, check


@case("search_by_sim3", ["orbm_search.hip/orbm_search_by_sim3"], weight=2)
def _():
    @functools.lru_cache(None)
    def scene():
        s = _tracking(2)
        rng = np.random.default_rng(2)
        v1 = ((s["src"] >= 0) & (rng.random(len(s["kps"])) < 0.85)).astype(np.uint8); mp1 = np.maximum(s["src"], 0)
        v2 = ((s["src2"] >= 0) & (rng.random(len(s["kps2"])) < 0.85)).astype(np.uint8); mp2 = np.maximum(s["src2"], 0)
        return s, v1, mp1, v2, mp2

    def run():
        from orb_slam2_e_amd import ORBmatcher, Points
        s, v1, mp1, v2, mp2 = scene()
        p1 = Points(v1, s["pos"][mp1], s["mp_desc"][mp1], min_distance=s["mind"][mp1], max_distance=s["maxd"][mp1])
        p2 = Points(v2, s["pos"][mp2], s["mp_desc"][mp2], min_distance=s["mind"][mp2], max_distance=s["maxd"][mp2])
        got = ORBmatcher(0.75, True).SearchBySim3Whole(_tracking_frame(2), _tracking_frame(2, second=True), _view(s), s["Tcw"], s["T2w"], s["s12"],
                                                       s["R12"], s["t12"], p1, p2, 7.5, want_queries=True)
        return _b(*got), None

    def check(out):
        import oracle
        s, v1, mp1, v2, mp2 = scene()
        ref = oracle.search_by_sim3_whole(s["kps"], s["desc"], s["kps2"], s["desc2"], s["bounds"], s["cam"], s["scale_factors"],
                                          s["log_scale_factor"], s["Tcw"], s["T2w"], s["s12"], s["R12"], s["t12"], v1, s["pos"][mp1],
                                          s["mind"][mp1], s["maxd"][mp1], s["mp_desc"][mp1], v2, s["pos"][mp2], s["mind"][mp2],
                                          s["maxd"][mp2], s["mp_desc"][mp2], 7.5)
        assert out[:4] == _b(*ref[:4])
    return run, check


@case("project_points", ["orbm_search.hip/orbm_project_points"])
def _():
    def run():
        import fuse_keyframes_scenes as S
        from orb_slam2_e_amd import ORBmatcher
        sc = _fuse_scene(); t = sc.targets[0]
        return _b(*ORBmatcher(0.8).project_points(1, sc.pos, sc.nrm, sc.mind, sc.maxd, t.R, t.t, t.Ow, S.cam_record(t.bounds), t.mbf, S.LOGSF, S.SF,
                                                  sc.th)), None

    def check(out):
        import fuse_keyframes_scenes as S
        sc = _fuse_scene(); t = sc.targets[0]
        assert out[0] == _b(S.project(t, sc.pos, sc.nrm, sc.mind, sc.maxd, sc.th, False)[0])[0]
    return run, check


@functools.lru_cache(None)
def _bow_pairs():
    import bow_pairs_scenes as B
    return [B.case_pair(1, 300, 320, 12), B.case_pair(2, 120, 150, 6), B.case_pair(3, 200, 90, 8)]


def _bow_pairs_case(name, sequential):
    @case(name, ["orbm_search.hip/bow_pairs_launch"] + (["orbm_search.hip/run_sequential"] if sequential else []), weight=2)
    def _():
        def run():
            from orb_slam2_e_amd import ORBmatcher
            m = ORBmatcher(0.7, True)
            if sequential:
                with forced_sequential():
                    got = m.frame_search_by_bow_pairs([p.args() for p in _bow_pairs()], True)
            else:
                got = m.frame_search_by_bow_pairs([p.args() for p in _bow_pairs()], True)
            return [b for g in got for b in _b(*g)], ORBmatcher.last_bow_pairs_waits()

        def check(out):
            ref = [b for p in _bow_pairs() for b in _b(*p.oracle(True, 0.7, True))]
            assert out == ref
        return run, check


_bow_pairs_case("bow_pairs", False)
_bow_pairs_case("bow_pairs_sequential", True)


# ------------------------------------------------------------------------------------------------------------- orbm_pose

def _track_bytes(got):
    res = got[0]
    return _b(np.array([res.tracked, res.search_used, res.nsearch, res.ngood, res.nmatches, res.nmatches_map], np.int64), *got[1:])


@case("track_motion_model", ["orbm_search.hip/run_sequential"], weight=2)
def _():
    def run():
        import track_reference as tr
        from orb_slam2_e_amd import ORBmatcher
        from test_gpu_track import _last
        s = _tracking(13, True)
        pc = tr.pose_camera(s)
        got = ORBmatcher(0.9, True).TrackWithMotionModel(_tracking_frame(13, True), _view(s), *pc, s["Tcw"], s["Tlw"], _last(tr.last_of(s)), 7.0, False)
        return _track_bytes(got), ORBmatcher.last_track_waits(), got

    def check(out, got):
        import track_reference as tr
        from orb_slam2_e_amd import ORBmatcher
        from test_gpu_track import _same_bits, _two_calls_mm
        s = _tracking(13, True)
        assert got[0].tracked == 1 and got[0].search_used == 1 and got[0].ngood > 20
        _same_bits(got, _two_calls_mm(ORBmatcher(0.9, True), _tracking_frame(13, True), s, tr.pose_camera(s), s["Tcw"], s["Tlw"], tr.last_of(s), 7.0, False))
    return run, check


@case("track_local_map", ["orbm_search.hip/run_sequential"], weight=2)
def _():
    def run():
        import track_reference as tr
        from orb_slam2_e_amd import ORBmatcher
        from test_gpu_track import _points
        s = _tracking(32, True)
        pts, bh, bpos, bt = tr.local_map_case(s)
        got = ORBmatcher(0.8, True).TrackLocalMap(_tracking_frame(32, True), _view(s), *tr.pose_camera(s), s["Tcw"], _points(pts), bh, bpos, bt, 3.0)
        return _track_bytes(got), ORBmatcher.last_track_waits(), got

    def check(out, got):
        import track_reference as tr
        from orb_slam2_e_amd import ORBmatcher
        from test_gpu_track import _same_bits, _two_calls_lm
        s = _tracking(32, True)
        pts, bh, bpos, bt = tr.local_map_case(s)
        assert got[0].ngood > 20
        _same_bits(got, _two_calls_lm(ORBmatcher(0.8, True), _tracking_frame(32, True), s, tr.pose_camera(s), s["Tcw"], pts, bh, bpos, bt, 3.0))
    return run, check


@functools.lru_cache(None)
def _pose_problems():
    import pose_only_scene as ps
    from test_gpu_pose import CASES as POSE_CASES
    out = []
    for name in ("stereo_50", "mono_50", "mixed_11"):       # scenes tests/test_gpu_pose.py holds to the restatement (margins asserted there)
        seed, n, sf, of, kw = POSE_CASES[name]
        out.append(ps.make_problem(seed, n, stereo_frac=sf, outlier_frac=of, **kw))
    return out


def _pose_agrees(p, got):
    """tests/test_gpu_pose.py's comparison with the restatement, its margins first"""
    import pose_only_oracle as po
    from test_gpu_pose import _agree, _margins_ok
    ref = po.run(p)
    _margins_ok(ref[3])
    _agree(p, got, ref)


def _pose_bytes(r):
    return _b(np.int32(r[0]), r[1], r[2], r[3])


@case("pose_optimization_batch", ["orbm_pose.hip/pose_host"])
def _():
    def run():
        import pose_only_scene as ps
        from orb_slam2_e_amd import pose_optimization_batch
        got = pose_optimization_batch(_pose_problems(), ps.CAM, ps.inv_level_sigma2())
        return [b for r in got for b in _pose_bytes(r)], None, got

    def check(out, got):
        for p, r in zip(_pose_problems(), got):
            _pose_agrees(p, r)
    return run, check


@case("frame_pose_optimization", ["orbm_pose.hip/orbm_frame_pose_optimization", "orbm_pose.hip/pose_host"])
def _():
    @functools.lru_cache(None)
    def frame():
        from orb_slam2_e_amd import Frame
        from orb_slam2_e_amd.extractor import KP_DTYPE
        p = _pose_problems()[0]
        k = np.zeros(len(p["octave"]), KP_DTYPE)
        k["x"], k["y"], k["octave"] = p["kp_xy"][:, 0], p["kp_xy"][:, 1], p["octave"]
        return Frame(k, np.zeros((len(k), 32), np.uint8), (-1e4, -1e4, 1e4, 1e4), p["uright"])

    def call(fr):
        from orb_slam2_e_amd import pose_optimization
        p = _pose_problems()[0]
        return pose_optimization(p["kp_xy"], p["octave"], p["uright"], p["has_mp"], p["mp_pos"], p["cam"], p["inv_sigma2"], p["Tcw"], frame=fr)

    def run():
        return _pose_bytes(call(frame())), None

    def check(out):
        """the restatement, and the resident form against the host-array form (tests/test_gpu_pose.py's equality)"""
        _pose_agrees(_pose_problems()[0], call(frame()))
        host = call(None)
        hm = _pose_problems()[0]["has_mp"] > 0
        res = call(frame())
        assert host[0] == res[0] and host[1].tobytes() == res[1].tobytes() and np.array_equal(host[2][hm], res[2][hm]) and bytes(host[3]) == bytes(res[3])
    return run, check


@case("pose_optimization_nr", ["orbm_pose_nr.hip/orbm_pose_optimization_nr"], weight=2)
def _():
    @functools.lru_cache(None)
    def scene():
        import pose_nr_bundle_oracle as nrb
        from orb_slam2_e_amd.fem import FEM_C3D6
        from test_gpu_pose_nr import SCENES, Case
        top, tris, g, _, K, u0, ids = nrb.fixture_problem("min", SCENES["min"])
        return Case(top, tris, FEM_C3D6, g, K, u0, ids)     # (the model, the graph and the restatement's result)

    def run():
        from orb_slam2_e_amd import pose as P
        from test_gpu_pose_nr import _bytes
        c = scene()
        got = P.pose_optimization_nr(c.fea, c.g, want_stats=True)
        two = [_bytes(r) for r in P.pose_optimization_nr_batch([c.fea, c.fea], [c.g, c.g], want_stats=True)]
        return _b(*(repr(x).encode() if not isinstance(x, bytes) else x for r in [_bytes(got)] + two for x in r)), None, got

    def check(out, got):
        """tests/test_gpu_pose_nr.py's parity with the restatement, on this call's result"""
        import copy
        from test_gpu_pose_nr import _parity
        c = copy.copy(scene())
        c.got = got
        _parity(c)
    return run, check


# ------------------------------------------------------------------------------------------- sim3, sim3opt, init, pnp, kfdb

@case("sim3_hypotheses", ["orbm_sim3.hip/orbm_sim3_hypotheses"])
def _():
    @functools.lru_cache(None)
    def problems():
        import sim3_scenes as S
        # tests/test_gpu_sim3.py's edge problems of n = 65 and n = 129 with H = 5
        return [S.problem(104, 65, 5, noise=1.0, outliers=0.3, name="edge_n65_H5"), S.problem(105, 129, 5, noise=1.0, outliers=0.3, name="edge_n129_H5")]

    def run():
        import sim3_scenes as S
        from orb_slam2_e_amd import Sim3Problem, sim3_hypotheses
        from orb_slam2_e_amd.sim3 import last_sim3_waits
        dev = [Sim3Problem(p["X1w"], p["X2w"], p["octave1"], p["octave2"], p["Tcw1"], p["Tcw2"], p["cam1"], p["cam2"], p["triples"], p["fix_scale"])
               for p in problems()]
        got = sim3_hypotheses(dev, S.SIGMA2)
        return [b for hyp, masks in got for b in _b(hyp, masks)], last_sim3_waits(), got

    def check(out, got):
        from test_gpu_sim3 import check_against_restatement
        for p, (hyp, masks) in zip(problems(), got):
            check_against_restatement(p, hyp, masks)
    return run, check


@case("optimize_sim3", ["orbm_sim3opt.hip/orbm_optimize_sim3"])
def _():
    @functools.lru_cache(None)
    def problems():
        import sim3_opt_scenes as S
        sc = S.gpu_scenes()             # the scenes tests/test_gpu_sim3_opt.py holds to the restatement: n = 65 free, n = 10 fixed scale
        return [next(p for p in sc if p["n"] == 65 and not p["fix_scale"]), next(p for p in sc if p["n"] == 10 and p["fix_scale"])]

    def run():
        import sim3_opt_scenes as S
        from orb_slam2_e_amd import sim3 as s3
        from test_cpu_sim3_opt import _dev
        got = s3.optimize_sim3([_dev(p) for p in problems()], S.INV_SIGMA2)
        return [b for r, kept in got for b in _b(r, kept)], s3.last_sim3_opt_waits(), got

    def check(out, got):
        """tests/test_gpu_sim3_opt.py's two comparisons with the restatement: (q, t, s) within M D_cpu; the integers and the kept
        flags equal where the restatement's own margins hold (no cut within M D_cpu th2 of th2, no trial with a tiny rho)"""
        import sim3_opt_oracle as so
        import sim3_opt_scenes as S
        from test_cpu_sim3_opt import M, _ints
        from test_gpu_sim3_opt import D_CPU, _vec
        compared = 0
        for p, (r, kept) in zip(problems(), got):
            ref = so.optimize(p, S.INV_SIGMA2)
            d = float(np.max(np.abs(_vec(r) - ref["res"].vec()) / np.abs(ref["res"].vec())))
            assert d <= M * D_CPU, (p["name"], d)
            cc, th2 = ref["cut_chi"], float(p["th2"])
            if np.sum(np.abs(cc[~np.isnan(cc)] - th2) < M * D_CPU * th2) or ref["trace"].small_rho:
                continue
            assert _ints(r) == _ints(ref["res"]) and np.array_equal(kept, ref["kept"]), p["name"]
            compared += 1
        assert compared >= 1
    return run, check


@functools.lru_cache(None)
def _init_scene():
    import init_scenes as S
    return next(s for s in S.edge_scenes() if s["name"] == "edge_n65_H5")       # one of the scenes tests/test_gpu_init.py compares


def _dict_bytes(d):
    return [b for k in sorted(d) for b in _b(d[k])]


@case("init_find_models", ["orbm_init.hip/orbm_init_find_models"])
def _():
    def run():
        from orb_slam2_e_amd import find_models, last_init_waits
        s = _init_scene()
        got = find_models(s["keys1"], s["keys2"], s["matches"], s["sets"], s.get("sigma", 1.0), per_hypothesis=True)      # a dict of arrays and scalars
        return _dict_bytes(got), last_init_waits(), got

    def check(out, got):
        from test_gpu_init import check_against_restatement
        check_against_restatement(_init_scene(), got)
    return run, check


@case("init_check_rt", ["orbm_init.hip/orbm_init_check_rt"])
def _():
    def run():
        import init_scenes as S
        from orb_slam2_e_amd import check_rt, last_init_waits
        from test_gpu_init import rt_scene
        s, inl, R, t = rt_scene(65, 4)
        d = check_rt(s["keys1"], s["keys2"], s["matches"], inl, S.K, R, t, np.float32(4.0))
        return _dict_bytes(d), last_init_waits(), d

    def check(out, d):
        from test_gpu_init import check_rt_against_restatement, rt_scene
        s, inl, R, t = rt_scene(65, 4)
        check_rt_against_restatement(s, d, inl, R, t, np.float32(4.0))
        assert d["ngood"][0] >= 0.7 * inl.sum()                 # the true motion triangulates the inliers
    return run, check


@case("pnp_hypotheses", ["orbm_pnp.hip/orbm_pnp_hypotheses"])
def _():
    @functools.lru_cache(None)
    def problems():
        import pnp_scenes as S
        return [S.problem(41, 65, 5), S.problem(43, 129, 5)]

    def run():
        import pnp_scenes as S
        from orb_slam2_e_amd import pnp
        dev = [pnp.PnpProblem(p["Xw"], p["uv"], p["octave"], p["cam"], p["sets"], p["min_inliers"], p["th2"]) for p in problems()]
        got = pnp.pnp_hypotheses(dev, S.SIGMA2)
        return [b for r in got for b in _b(*r)], pnp.last_pnp_waits(), got

    def check(out, got):
        from test_gpu_pnp import _assert_equal
        for p, r in zip(problems(), got):
            _assert_equal(p, r)
    return run, check


@functools.lru_cache(None)
def _kfdb_scene():
    """70 BowVectors of three places, a query, the slots that get erased and the slots that are scored"""
    import kfdb_scenes as S
    rng = np.random.default_rng(7)
    pl = S.Places(rng, 1000, 3, 120)
    return [pl.bow(int(rng.integers(3)), 60, 0.7) for _ in range(70)], pl.bow(1, 60, 0.9), (3, 64), [s for s in range(70) if s not in (3, 64)][::3]


def _kfdb_build():
    from orb_slam2_e_amd import KeyFrameDatabase
    bows, _, erased, _ = _kfdb_scene()
    db = KeyFrameDatabase(1000)
    slots = [db.add(b) for b in bows]
    for s in erased:
        db.erase(s)
    return db, slots


_kfdb_resident = functools.lru_cache(None)(_kfdb_build)       # built once, in front of every fill: its calls stage the query only


@functools.lru_cache(None)
def _kfdb_reference():
    import kfdb_reference as R
    bows, _, erased, _ = _kfdb_scene()
    ref = R.ReferenceDatabase(1000)
    slots = [ref.add(b) for b in bows]
    for s in erased:
        ref.erase(s)
    return ref, slots


@case("kfdb_add_erase", ["orbm_kfdb.hip/orbm_kfdb_add", "orbm_kfdb.hip/orbm_kfdb_erase"])
def _():
    def run():
        """a database filled and thinned (the first add meets the arena as the test left it), read back through one query"""
        db, slots = _kfdb_build()
        return _b(np.array(slots, np.int32), *db.query(_kfdb_scene()[1])), None

    def check(out):
        ref, slots = _kfdb_reference()
        assert out == _b(np.array(slots, np.int32), *ref.shared(_kfdb_scene()[1]))
    return run, check


@case("kfdb_query", ["orbm_kfdb.hip/orbm_kfdb_query"])
def _():
    def run():
        db, _ = _kfdb_resident()
        got = db.query(_kfdb_scene()[1])
        return _b(*got), db.last_waits()

    def check(out):
        wc, wf, ws = _kfdb_reference()[0].shared(_kfdb_scene()[1])
        assert out == _b(wc, wf, ws) and (wc > 0).sum() > 10 and (wc < 0).sum() == 2
    return run, check


@case("kfdb_score", ["orbm_kfdb.hip/orbm_kfdb_score"])
def _():
    def run():
        db, _ = _kfdb_resident()
        _, q, _, listed = _kfdb_scene()
        got = db.score(q, listed)
        return _b(got), db.last_waits()

    def check(out):
        _, q, _, listed = _kfdb_scene()
        assert out == _b(_kfdb_reference()[0].score(q, listed)) and len(listed) > 20
    return run, check


# ----------------------------------------------------------------------------------------------------------- orbm_triang

@functools.lru_cache(None)
def _triang_args():
    from test_gpu_match import _triangulation_case
    return _triangulation_case(0, False)


@case("match_triangulation", ["orbm_triang.hip/triang_host_arrays"])
def _():
    def run():
        from orb_slam2_e_amd import ORBmatcher
        args, os_ = _triang_args()
        return _b(*ORBmatcher(0.6, False).match_triangulation(*args, bOnlyStereo=os_)), None

    def check(out):
        import oracle
        args, os_ = _triang_args()
        assert out == _b(*oracle.match_triangulation(*args, only_stereo=os_))
    return run, check


@case("frame_search_for_triangulation", ["orbm_triang.hip/orbm_frame_search_for_triangulation"])
def _():
    @functools.lru_cache(None)
    def scene():
        import oracle
        from orb_slam2_e_amd import Frame
        (k1, d1, k2, d2, _, _, mp1, mp2, s1, s2, F12, ex, ey, sf, sg), _ = _triang_args()
        rng = np.random.default_rng(100)
        n = len(k1)
        node1 = rng.integers(0, 45, n) * 3 + 7
        node2 = np.where(rng.random(n) < 0.9, node1, rng.integers(0, 50, n) * 3 + 7)
        k1 = k1.copy(); k2 = k2.copy()
        k1["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        k2["angle"] = np.where(rng.random(n) < 0.8, (k1["angle"] + rng.normal(0, 4, n)) % 360, rng.uniform(0, 360, n)).astype(np.float32)
        fv1, fv2 = oracle.feature_vector(node1, rng.random(n) < 0.95), oracle.feature_vector(node2, rng.random(n) < 0.95)
        z = np.zeros(n, bool)
        return (Frame(k1, d1, BOUNDS), Frame(k2, d2, BOUNDS)), (k1, d1, fv1, mp1, z, k2, d2, fv2, mp2, z, F12, ex, ey, sf, sg)

    def run():
        from orb_slam2_e_amd import ORBmatcher
        (f1, f2), (k1, d1, fv1, mp1, z, k2, d2, fv2, mp2, _, F12, ex, ey, sf, sg) = scene()
        pairs, nm, m12 = ORBmatcher(0.6, True).frame_search_for_triangulation(f1, fv1, mp1, f2, fv2, mp2, F12, ex, ey, sf, sg, False)
        return _b(np.asarray(pairs, np.int32), np.int32(nm), m12), None

    def check(out):
        import oracle
        _, a = scene()
        r12, rn = oracle.search_for_triangulation(*a, False, True)
        assert out[1:] == _b(np.int32(rn), r12) and rn > 30
    return run, check


@case("create_new_map_points", ["orbm_triang.hip/orbm_create_new_map_points"], weight=2)
def _():
    @functools.lru_cache(None)
    def scene():
        import create_points_scenes as S
        from test_gpu_create_points import DeviceScene
        s = S.random_scene(7, 65, 2)
        return s, DeviceScene(s)

    def run():
        from orb_slam2_e_amd import ORBmatcher
        s, d = scene()
        got = d.run()
        return _b(got.match12, got.status, got.x3d, got.counts, np.int32(got.nnew)), ORBmatcher.last_create_points_waits(), got

    def check(out, got):
        """the first neighbour's matches against the search it chains (tests/test_gpu_create_points.py's first equality)"""
        from orb_slam2_e_amd import ORBmatcher
        s, d = scene()
        cur, nb = s["cur"], s["neigh"][0]
        _, _, m12 = ORBmatcher(0.6, False).frame_search_for_triangulation(d.cur.frame, cur["fv"], cur["has"], d.neigh[0].frame, nb["fv"], nb["has"],
                                                                         nb["F12"], nb["ex"], nb["ey"], s["sf"], s["sg"], False)
        assert np.array_equal(got.match12[0], m12) and got.nnew > 0
    return run, check


# ------------------------------------------------------------------------------------------------------------ the table

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FILLS = [("zero", 0x00000000, 0), ("one", 0x00000001, 0), ("next_generation", 0, 1), ("nan", 0x7FC00000, 0), ("minus_one", 0xFFFFFFFF, 0)]


def fill_workspaces(word, as_next_generation=0):
    """orbm_debug_fill_workspaces -> (workspaces filled, pooled frame blocks filled)"""
    from orb_slam2_e_amd._lib import check
    nw, nb = C.c_int(-1), C.c_int(-1)
    check(_lib().orbm_debug_fill_workspaces(word, as_next_generation, C.byref(nw), C.byref(nb)))
    return nw.value, nb.value


def run_case(c):
    """(outputs, waits, extra for check)"""
    r = c.run()
    return r[0], r[1], r[2:]


def tagged_sites():
    return {s for c in CASES for s in c.sites}
