"""Host-side mirror of the ORBmatcher data plane over the C-ABI (ctypes).

Constants and semantics follow include/ORBmatcher.h:37-111 and
src/ORBmatcher.cc:37-40 (TH_HIGH=95, TH_LOW=45, TH_RELOC=60, HISTO_LENGTH=30).
"""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr as _p




class ORBmatcher:
    # src/ORBmatcher.cc:37-40
    TH_HIGH = 95
    TH_LOW = 45
    TH_RELOC = 60
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio = np.float32(nnratio)
        self.mbCheckOrientation = checkOri
        self._L = lib()

    @staticmethod
    def DescriptorDistance(a, b):
        """ORBmatcher::DescriptorDistance for one pair (runs the device kernel)."""
        return int(ORBmatcher.hamming_matrix(np.reshape(a, (1, 32)), np.reshape(b, (1, 32)))[0, 0])

    @staticmethod
    def hamming_matrix(A, B):
        L = lib()
        A = np.ascontiguousarray(A, np.uint8); B = np.ascontiguousarray(B, np.uint8)
        out = np.zeros((len(A), len(B)), np.uint16)
        check(L.orbm_hamming_matrix(_p(A), len(A), _p(B), len(B), _p(out)))
        return out

    ALLPAIRS_AUTO, ALLPAIRS_POPCOUNT, ALLPAIRS_MFMA = 0, 1, 2

    @staticmethod
    def set_allpairs_kernel(kind):
        """orbm_set_allpairs_kernel: which kernel the all-pairs matchers launch (process-wide); returns the previous one."""
        prev = lib().orbm_set_allpairs_kernel(int(kind))
        if prev < 0:
            raise ValueError("unknown all-pairs kernel kind")
        return prev

    def match_bruteforce(self, A, B):
        A = np.ascontiguousarray(A, np.uint8); B = np.ascontiguousarray(B, np.uint8)
        nA = len(A)
        best = np.zeros(nA, np.int32); second = np.zeros(nA, np.int32); idx = np.zeros(nA, np.int32)
        check(self._L.orbm_match_bruteforce(_p(A), nA, _p(B), len(B), _p(best), _p(second), _p(idx)))
        return best, second, idx

    def match_candidates(self, A, B, cand_off, cand_idx):
        A = np.ascontiguousarray(A, np.uint8); B = np.ascontiguousarray(B, np.uint8)
        off = np.ascontiguousarray(cand_off, np.int32); ci = np.ascontiguousarray(cand_idx, np.int32)
        nA = len(A)
        best = np.zeros(nA, np.int32); second = np.zeros(nA, np.int32); idx = np.zeros(nA, np.int32)
        check(self._L.orbm_match_candidates(_p(A), nA, _p(B), len(B), _p(off), _p(ci), _p(best), _p(second), _p(idx)))
        return best, second, idx

    def filter(self, best, second, idx, th=None):
        th = self.TH_LOW if th is None else th
        m = np.zeros(len(best), np.int32)
        n = C.c_int(0)
        check(self._L.orbm_match_filter(len(best), _p(np.ascontiguousarray(best, np.int32)),
                                        _p(np.ascontiguousarray(second, np.int32)),
                                        _p(np.ascontiguousarray(idx, np.int32)), th, self.mfNNratio,
                                        _p(m), C.byref(n)))
        return m, n.value

    def match_batch_device(self, desc_dev, counts_dev, cap, pair_a_dev, pair_b_dev, npairs,
                           best_dev, second_dev, idx_dev, match12_dev, nmatch_dev, th=None, stream=None):
        th = self.TH_LOW if th is None else th
        check(self._L.orbm_match_batch_dev(desc_dev, counts_dev, cap, pair_a_dev, pair_b_dev, npairs, th, self.mfNNratio, best_dev,
                                           second_dev, idx_dev, match12_dev, nmatch_dev, stream))

    def match_triangulation(self, kps1, desc1, kps2, desc2, cand_off, cand_idx, has_mp1, has_mp2, stereo1, stereo2,
                            F12, ex, ey, scale_factors2, level_sigma2, bOnlyStereo=False):
        """Inner loop of ORBmatcher::SearchForTriangulation (ORBmatcher.cc:892-990).
        Returns (vMatches12, bestDist); rotation histogram / pair list stay on the host."""
        kps1 = np.ascontiguousarray(kps1); kps2 = np.ascontiguousarray(kps2)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        off = np.ascontiguousarray(cand_off, np.int32); ci = np.ascontiguousarray(cand_idx, np.int32)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8)
        m1, m2, s1, s2 = u8(has_mp1), u8(has_mp2), u8(stereo1), u8(stereo2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sc = np.ascontiguousarray(scale_factors2, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
        n1 = len(kps1)
        m12 = np.zeros(n1, np.int32); bd = np.zeros(n1, np.int32)
        check(self._L.orbm_match_triangulation(_p(kps1), _p(d1), n1, _p(kps2), _p(d2), len(kps2), _p(off), _p(ci), _p(m1),
                                               _p(m2), _p(s1), _p(s2), 1 if bOnlyStereo else 0, _p(F), ex, ey, _p(sc),
                                               _p(sg), len(sc), _p(m12), _p(bd)))
        return m12, bd

    def SearchForTriangulation(self, kps1, desc1, fv1, has_mp1, stereo1, kps2, desc2, fv2, has_mp2, stereo2, F12, ex, ey,
                               scale_factors2, level_sigma2, bOnlyStereo=False):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:858-1024): FeatureVector co-iteration into per-keypoint
        candidate lists (host), the gated loop on the device, rotation histogram + ComputeThreeMaxima + pair list (host).
        fv = (nodes ascending, off, items).  Returns (vMatchedPairs as an (m, 2) array, nmatches, vMatches12)."""
        n1, n2 = len(kps1), len(kps2)
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8)
        k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        (nd1, of1, it1), (nd2, of2, it2) = (tuple(i32(a) for a in fv) for fv in (fv1, fv2))
        h1, h2, s1, s2 = u8(has_mp1), u8(has_mp2), u8(stereo1), u8(stereo2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sf = np.ascontiguousarray(scale_factors2, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
        m12 = np.full(n1, -1, np.int32); nm = C.c_int(0)
        check(self._L.orbm_search_for_triangulation(_p(k1), _p(d1), n1, _p(nd1), _p(of1), _p(it1), len(nd1), _p(h1), _p(s1),
                                                    _p(k2), _p(d2), n2, _p(nd2), _p(of2), _p(it2), len(nd2), _p(h2), _p(s2),
                                                    int(bool(bOnlyStereo)), _p(F), float(ex), float(ey), _p(sf), _p(sg), len(sf),
                                                    int(self.mbCheckOrientation), _p(m12), C.byref(nm)))
        i1 = np.nonzero(m12 >= 0)[0]
        return np.stack([i1, m12[i1]], 1), nm.value, m12

    @staticmethod
    def feature_vector_candidates(n1, fv1, fv2):
        """The co-iteration of two FeatureVectors (ORBmatcher.cc:881-891, 1004-1012) as per-keypoint candidate lists: a
        keypoint of frame 1 whose node also exists in frame 2 gets that node's members of frame 2, in their order.
        fv = (nodes ascending, off, items).  Returns (cand_off[n1 + 1], cand_idx)."""
        nodes1, off1, items1 = (np.asarray(a, np.int64) for a in fv1); nodes2, off2, items2 = (np.asarray(a, np.int64) for a in fv2)
        _, ia, ib = np.intersect1d(nodes1, nodes2, assume_unique=True, return_indices=True)
        len1 = off1[ia + 1] - off1[ia]; len2 = off2[ib + 1] - off2[ib]
        tot1 = int(len1.sum())
        seg = np.repeat(off1[ia], len1) + (np.arange(tot1) - np.repeat(np.cumsum(len1) - len1, len1))
        members1 = items1[seg]                                      # keypoints of frame 1 that have candidates
        cnt = np.zeros(n1, np.int64); start2 = np.zeros(n1, np.int64)
        cnt[members1] = np.repeat(len2, len1); start2[members1] = np.repeat(off2[ib], len1)
        cand_off = np.zeros(n1 + 1, np.int32); cand_off[1:] = np.cumsum(cnt)
        tot = int(cand_off[-1])
        pos = np.repeat(start2, cnt) + (np.arange(tot) - np.repeat(cand_off[:-1].astype(np.int64), cnt))
        return cand_off, items2[pos].astype(np.int32)

    @staticmethod
    def ComputeThreeMaxima(hist):
        """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1802-1843) on the bin sizes -> the bins that stay."""
        max1 = max2 = max3 = 0; ind1 = ind2 = ind3 = -1
        for i, s in enumerate(int(x) for x in hist):
            if s > max1: max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
            elif s > max2: max3, max2, ind3, ind2 = max2, s, ind2, i
            elif s > max3: max3, ind3 = s, i
        if max2 < np.float32(0.1) * np.float32(max1): ind2 = ind3 = -1
        elif max3 < np.float32(0.1) * np.float32(max1): ind3 = -1
        return [i for i in (ind1, ind2, ind3) if i >= 0]

    WQ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("r", "<f4"), ("xr", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")])

    def search_window(self, queries, qdesc, kps, desc, bounds, skip=None, uright=None, init_dist=256):
        """GetFeaturesInArea + best/second-with-levels (ORBmatcher.cc:69-118).
        queries: array of WQ_DTYPE; bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY).
        Returns best, best_level, second, second_level, idx."""
        q = np.ascontiguousarray(queries, self.WQ_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
        kps = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
        nq = len(q)
        outs = [np.zeros(nq, np.int32) for _ in range(5)]
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        ur = np.ascontiguousarray(uright, np.float32) if uright is not None else None
        check(self._L.orbm_search_window(_p(q), _p(qd), nq, _p(kps), _p(d), len(kps), _p(sk) if sk is not None else None,
                                         _p(ur) if ur is not None else None, *[float(b) for b in bounds], init_dist,
                                         *[_p(o) for o in outs]))
        return tuple(outs)

    def search_projection(self, queries, qdesc, qangle, qtakes, kps, desc, bounds, occupied=None, uright=None, th_accept=None,
                          ratio_same_level=False):
        """The SearchByProjection family as a whole loop (ORBmatcher.cc:46-132, :491-604, :1529-1800): in-loop
        assignment, acceptance, rotation check (self.mbCheckOrientation).  Returns (match_kp, match_q, nmatches):
        match_kp[j] = query assigned to keypoint j (-1 untouched, -2 cleared by the rotation check)."""
        q = np.ascontiguousarray(queries, self.WQ_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
        qa = np.ascontiguousarray(qangle, np.float32) if qangle is not None else None
        qt = np.ascontiguousarray(qtakes, np.uint8) if qtakes is not None else None
        kps = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
        oc = np.ascontiguousarray(occupied, np.uint8) if occupied is not None else None
        ur = np.ascontiguousarray(uright, np.float32) if uright is not None else None
        nq, n = len(q), len(kps)
        mk = np.zeros(n, np.int32); mq = np.zeros(nq, np.int32); nm = C.c_int(0)
        opt = lambda a: _p(a) if a is not None else None
        check(self._L.orbm_search_projection(_p(q), _p(qd), opt(qa), opt(qt), nq, _p(kps), _p(d), n, opt(oc), opt(ur),
                                             *[float(b) for b in bounds], self.TH_HIGH if th_accept is None else int(th_accept),
                                             self.mfNNratio, int(ratio_same_level), int(self.mbCheckOrientation),
                                             _p(mk), _p(mq), C.byref(nm)))
        return mk, mq, nm.value

    def search_fuse(self, queries, qdesc, kps, desc, bounds, uright=None, inv_level_sigma2=None):
        """Candidate loop of ORBmatcher::Fuse (ORBmatcher.cc:1092-1146) -> (bestDist, bestIdx) per projected point."""
        q = np.ascontiguousarray(queries, self.WQ_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
        kps = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
        ur = np.ascontiguousarray(uright, np.float32) if uright is not None else None
        sg = np.ascontiguousarray(inv_level_sigma2, np.float32) if inv_level_sigma2 is not None else None
        best = np.zeros(len(q), np.int32); idx = np.zeros(len(q), np.int32)
        check(self._L.orbm_search_fuse(_p(q), _p(qd), len(q), _p(kps), _p(d), len(kps), _p(ur) if ur is not None else None,
                                       _p(sg) if sg is not None else None, len(sg) if sg is not None else 0,
                                       *[float(b) for b in bounds], _p(best), _p(idx)))
        return best, idx

    def SearchBySim3(self, q12, qdesc1, kps2, desc2, q21, qdesc2, kps1, desc1, bounds):
        """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1303-1527) over projected points (r < 0 = skipped point): two
        independent window searches (levels [l-1, l], <= TH_HIGH) and the agreement check (:1509-1524).
        Returns (match12, nFound)."""
        b1, _, _, _, i1 = self.search_window(q12, qdesc1, kps2, desc2, bounds, None, None, 2**31 - 1)
        b2, _, _, _, i2 = self.search_window(q21, qdesc2, kps1, desc1, bounds, None, None, 2**31 - 1)
        m1 = np.where((i1 >= 0) & (b1 <= self.TH_HIGH), i1, -1); m2 = np.where((i2 >= 0) & (b2 <= self.TH_HIGH), i2, -1)
        ok = m1 >= 0
        agree = np.zeros(len(m1), bool)
        agree[ok] = m2[m1[ok]] == np.nonzero(ok)[0]
        out = np.where(agree, m1, -1).astype(np.int32)
        return out, int(agree.sum())

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, vbPrevMatched, bounds, windowSize=10):
        """ORBmatcher::SearchForInitialization (ORBmatcher.cc:606-721).  kps = mvKeysUn of F1 / F2, bounds = F2's
        grid bounds.  Returns (vnMatches12, updated vbPrevMatched, nmatches)."""
        k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        pv = np.array(vbPrevMatched, np.float32, copy=True).reshape(-1, 2)
        m12 = np.zeros(len(k1), np.int32); nm = C.c_int(0)
        check(self._L.orbm_search_for_initialization(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), _p(pv),
                                                     *[float(b) for b in bounds], int(windowSize), self.mfNNratio,
                                                     int(self.mbCheckOrientation), _p(m12), C.byref(nm)))
        return m12, pv, nm.value

    def SearchByBoW(self, fv1, valid1, desc1, angle1, fv2, valid2, desc2, angle2, kf_kf=False):
        """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:360-489; kf_kf=False) or
        SearchByBoW(KeyFrame*, KeyFrame*, ...) (:723-856; kf_kf=True).  fv = feature_vector_arrays(...) of each
        side, valid = "owns a good MapPoint" masks (valid2 only for the KeyFrame form), angle = mvKeysUn angles.
        Returns (match12, match21, nmatches)."""
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        a1 = np.ascontiguousarray(angle1, np.float32); a2 = np.ascontiguousarray(angle2, np.float32)
        nodes1, off1, it1 = [i32(a) for a in fv1]; nodes2, off2, it2 = [i32(a) for a in fv2]
        v1 = np.ascontiguousarray(valid1, np.uint8)
        v2 = np.ascontiguousarray(valid2, np.uint8) if kf_kf else None
        n1, n2 = len(d1), len(d2)
        m12 = np.zeros(n1, np.int32); m21 = np.zeros(n2, np.int32); nm = C.c_int(0)
        check(self._L.orbm_search_by_bow(_p(nodes1), _p(off1), _p(it1), len(nodes1), _p(v1), _p(d1), _p(a1), n1,
                                         _p(nodes2), _p(off2), _p(it2), len(nodes2), _p(v2) if v2 is not None else None, _p(d2),
                                         _p(a2), n2, self.TH_LOW, int(kf_kf), self.mfNNratio,
                                         int(self.mbCheckOrientation), _p(m12), _p(m21), C.byref(nm)))
        return m12, m21, nm.value

    CAM_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("min_x", "<i4"), ("max_x", "<i4"),
                          ("min_y", "<i4"), ("max_y", "<i4"), ("gminx", "<f4"), ("gminy", "<f4"), ("gmaxx", "<f4"), ("gmaxy", "<f4")])

    def SearchByProjectionMap(self, kps, desc, has_mp, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, Rcw, tcw, cam,
                              scale_factors, th=1.0):
        """The fork's SearchByProjection(Frame&, Map*, Rcw, tcw, ...) (ORBmatcher.cc:134-222).
        Returns (vMatchedMPs as indices or -1, nmatches, proj[m,4])."""
        kps = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
        hm = np.ascontiguousarray(has_mp, np.uint8)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos), f32(mp_normal), f32(mp_min_dist), f32(mp_max_dist)
        md = np.ascontiguousarray(mp_desc, np.uint8)
        R = np.ascontiguousarray(Rcw, np.float64).reshape(9); t = np.ascontiguousarray(tcw, np.float64).reshape(3)
        cam = np.ascontiguousarray(cam, self.CAM_DTYPE).reshape(1)
        sc = f32(scale_factors)
        n, m = len(kps), len(pos)
        matched = np.zeros(n, np.int32); proj = np.zeros((m, 4), np.float32); nm = C.c_int(0)
        check(self._L.orbm_search_by_projection_map(_p(kps), _p(d), n, _p(hm), _p(pos), _p(nrm), _p(mn), _p(mx), _p(md), m,
                                                    _p(R), _p(t), _p(cam), _p(sc), len(sc), th, self.mfNNratio,
                                                    self.TH_RELOC, _p(matched), C.byref(nm), _p(proj)))
        return matched, nm.value, proj

    PROJ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("view_cos", "<f4"), ("dist", "<f4"), ("level", "<i4"),
                           ("visible", "<i4")])
    PROJECT_FRUSTUM, PROJECT_FUSE, PROJECT_FUSE_SIM3 = 0, 1, 2

    def project_points(self, mode, mp_pos, mp_normal, mp_min_distance, mp_max_distance, Rcw, tcw, Ow, cam, mbf, log_scale_factor,
                       scale_factors, th=1.0, viewing_cos_limit=0.5):
        """orbm_project_points: Frame::isInFrustum + MapPoint::PredictScale (Frame.cc:284-340, MapPoint.cc:464-480;
        mode PROJECT_FRUSTUM) or the projection block of ORBmatcher::Fuse (ORBmatcher.cc:1053-1094 / :1212-1250) for all
        map points at once.  Returns (projected[PROJ_DTYPE], window queries[WQ_DTYPE])."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos), f32(mp_normal), f32(mp_min_distance), f32(mp_max_distance)
        R, t, O = f32(Rcw).reshape(9), f32(tcw).reshape(3), f32(Ow).reshape(3)
        cam = np.ascontiguousarray(cam, self.CAM_DTYPE).reshape(1)
        sc = f32(scale_factors)
        m = len(pos)
        out = np.zeros(m, self.PROJ_DTYPE); q = np.zeros(m, self.WQ_DTYPE)
        check(self._L.orbm_project_points(int(mode), _p(pos), _p(nrm), _p(mn), _p(mx), m, _p(R), _p(t), _p(O), _p(cam), float(mbf),
                                          float(viewing_cos_limit), float(log_scale_factor), _p(sc), len(sc), float(th), _p(out), _p(q)))
        return out, q

    def Fuse(self, kps, desc, uright, bounds, inv_level_sigma2, vpMapPoints, mp_pos, mp_normal, mp_min_distance, mp_max_distance,
             mp_desc, Rcw, tcw, Ow, cam, mbf, log_scale_factor, scale_factors, th, map_ops, sim3=False):
        """ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) as a whole (ORBmatcher.cc:1026-1176; sim3=True: the
        projection and candidate loop of the Sim3 form, :1178-1301, whose map update differs -- see fuse_replay):
        projection of every listed map point and the gated candidate loop on the device, then the reference's loop tail
        on the host in list order.  vpMapPoints[i] = map point handle or -1 (NULL entry); mp_* arrays are indexed by i.
        map_ops: is_bad(h), is_in_keyframe(h), slot_owner(idx) -> handle or -1, observations(h), replace(dead, heir),
        add(h, idx); the Sim3 form needs already_found(h) (spAlreadyFound, a snapshot) and record_replace(i, h) instead of
        is_in_keyframe / observations / replace.  Returns nFused."""
        mode = self.PROJECT_FUSE_SIM3 if sim3 else self.PROJECT_FUSE
        proj, q = self.project_points(mode, mp_pos, mp_normal, mp_min_distance, mp_max_distance, Rcw, tcw, Ow, cam, mbf,
                                      log_scale_factor, scale_factors, th)
        best, idx = self.search_fuse(q, mp_desc, kps, desc, bounds, uright, None if sim3 else inv_level_sigma2)
        if sim3:
            return self.fuse_replay_sim3(vpMapPoints, proj["visible"], best, idx, map_ops)
        return self.fuse_replay(vpMapPoints, proj["visible"], best, idx, map_ops)

    def fuse_replay_sim3(self, vpPoints, visible, best, idx, map_ops):
        """The tail of the Sim3 form (ORBmatcher.cc:1194-1205 skips, :1279-1296 update): the "already found" test reads the
        snapshot of the key frame's map points taken before the loop -- map_ops.already_found(h) must answer from that
        snapshot (KeyFrame::GetMapPoints at call time), not from the state the loop is changing; a taken slot is only
        recorded, map_ops.record_replace(i, h_in_kf) (vpReplacePoint[i] = pMPinKF); a free slot gets the point."""
        nFused = 0
        for i, h in enumerate(vpPoints):
            if h < 0 or map_ops.is_bad(h) or map_ops.already_found(h):
                continue
            if not visible[i] or idx[i] < 0:
                continue
            if best[i] <= self.TH_LOW:
                other = map_ops.slot_owner(int(idx[i]))
                if other >= 0:
                    if not map_ops.is_bad(other):
                        map_ops.record_replace(i, other)
                else:
                    map_ops.add(h, int(idx[i]))
                nFused += 1
        return nFused

    def fuse_replay(self, vpMapPoints, visible, best, idx, map_ops):
        """The tail of the Fuse loop (ORBmatcher.cc:1046-1053 skips, :1149-1170 update) in the list's order: the candidate
        search of a point does not depend on the map state, the skips and the update do."""
        nFused = 0
        for i, h in enumerate(vpMapPoints):
            if h < 0 or map_ops.is_bad(h) or map_ops.is_in_keyframe(h):
                continue
            if not visible[i] or idx[i] < 0:
                continue
            if best[i] <= self.TH_LOW:
                other = map_ops.slot_owner(int(idx[i]))
                if other >= 0:
                    if not map_ops.is_bad(other):
                        if map_ops.observations(other) > map_ops.observations(h):
                            map_ops.replace(h, other)       # pMP->Replace(pMPinKF)
                        else:
                            map_ops.replace(other, h)       # pMPinKF->Replace(pMP)
                else:
                    map_ops.add(h, int(idx[i]))             # AddObservation + AddMapPoint
                nFused += 1
        return nFused

    MAX_FUSE_TARGETS, MAX_FUSE_POINTS, MAX_FUSE_PAIRS = 128, 65536, 4194304

    def fuse_keyframes_rows(self, targets, mp_pos, mp_normal, mp_min_distance, mp_max_distance, mp_desc, log_scale_factor, scale_factors,
                            inv_level_sigma2, th, active=None, sim3=False, want_projected=True):
        """orbm_fuse_keyframes: the device half of ORBmatcher::Fuse (projection + gated candidate loop) for every (target
        keyframe, list entry) pair in one call.  targets = a sequence of FuseTarget; active = [K][m] bytes or None.  Row k of
        the results is what project_points + frame_search_fuse return for target k alone.  Returns (best[K, m], idx[K, m],
        projected[K, m] of PROJ_DTYPE or None)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos).reshape(-1, 3), f32(mp_normal).reshape(-1, 3), f32(mp_min_distance), f32(mp_max_distance)
        d = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        K, m = len(targets), len(pos)
        arr = (_CFuseTarget * max(K, 1))(*[t.c for t in targets])
        sc = f32(scale_factors)
        sg = f32(inv_level_sigma2) if inv_level_sigma2 is not None else None
        act = np.ascontiguousarray(active, np.uint8).reshape(K, m) if active is not None else None
        best = np.zeros((K, m), np.int32); idx = np.zeros((K, m), np.int32)
        proj = np.zeros((K, m), self.PROJ_DTYPE) if want_projected else None
        opt = lambda a: _p(a) if a is not None and a.size else None
        check(self._L.orbm_fuse_keyframes(arr if K else None, K, int(sim3), opt(pos), opt(nrm), opt(mn), opt(mx), opt(d), m, opt(act),
                                          float(th), float(log_scale_factor), _p(sc), _p(sg) if sg is not None else None, len(sc),
                                          opt(best), opt(idx), opt(proj) if proj is not None else None))
        return best, idx, proj

    @staticmethod
    def last_fuse_keyframes_rows_waits():
        """orbm_debug_last_fuse_keyframes_waits: host waits of the last orbm_fuse_keyframes of this process (1 when it launched)."""
        return lib().orbm_debug_last_fuse_keyframes_waits()

    _last_fuse_keyframes = {"waits": 0, "refreshes": 0}

    @staticmethod
    def last_fuse_keyframes_waits():
        """Host waits of the last fuse_keyframes (the whole loop) of this process: 1 + its refreshes when the first call launched."""
        return ORBmatcher._last_fuse_keyframes["waits"]

    @staticmethod
    def last_fuse_keyframes_refreshes():
        return ORBmatcher._last_fuse_keyframes["refreshes"]

    def fuse_keyframes(self, targets, vpMapPoints, mp_pos, mp_normal, mp_min_distance, mp_max_distance, mp_desc, log_scale_factor,
                       scale_factors, inv_level_sigma2, th, map_ops, sim3=False, candidates=None):
        """The loop `for pKFi in targets: matcher.Fuse(pKFi, vpMapPoints)` of LocalMapping::SearchInNeighbors
        (LocalMapping.cc:550-558) as a whole, or with sim3=True the loop of LoopClosing::SearchAndFuse (LoopClosing.cc:587-613)
        over the Sim3 form: one device call for all K x m pairs, then the reference's loop tails (fuse_replay /
        fuse_replay_sim3) on the host, target by target in list order.  Returns nFused per target.

        MapPoint::Replace ends with ComputeDistinctiveDescriptors on the heir (MapPoint.cc:275), so the descriptor of a list
        entry can change between two targets: after target k the rows of the LATER targets are computed again, in one more call,
        for the entries that were reported as an heir, are not bad and whose map_ops.descriptor(h) differs bytewise from the
        bytes their rows were computed with.  The result is the sequential loop's.

        map_ops: what fuse_replay / fuse_replay_sim3 ask for, answered for the CURRENT target, plus begin_target(k) (the Sim3
        form takes its spAlreadyFound snapshot here), end_target(k, report) (the Sim3 caller runs its Replace loop of
        LoopClosing.cc:604-611 here and calls report(i) for every list index i it replaced into), descriptor(h) (32 bytes) and,
        for the mask, in_target(h, k): IsInKeyFrame(target k) -- in the Sim3 form: h is among target k's map points -- at the
        time of the call.  The mask is an optimisation only: the tails test every skip again at their own time.
        candidates (optional): a callable (targets, points, desc, active) -> (best, idx, visible), each [len(targets)][len(points)],
        standing in for the device; points = list indices, desc = their descriptors, active = [len(targets)][len(points)]."""
        lst = np.ascontiguousarray(vpMapPoints, np.int32)
        K, m = len(targets), len(lst)
        desc = np.array(mp_desc, np.uint8).reshape(m, 32).copy()      # the bytes the rows were computed with
        stats = {"waits": 0, "refreshes": 0}
        if candidates is None:
            f32 = lambda a: np.ascontiguousarray(a, np.float32)
            pos, nrm, mn, mx = f32(mp_pos).reshape(m, 3), f32(mp_normal).reshape(m, 3), f32(mp_min_distance), f32(mp_max_distance)

            def candidates(tg, points, d, act):
                b, ix, pr = self.fuse_keyframes_rows(tg, pos[points], nrm[points], mn[points], mx[points], d, log_scale_factor,
                                                     scale_factors, inv_level_sigma2, th, act, sim3)
                stats["waits"] += self.last_fuse_keyframes_rows_waits()
                return b, ix, pr["visible"]
        else:
            inner = candidates

            def candidates(tg, points, d, act):
                stats["waits"] += 1
                return inner(tg, points, d, act)
        # mask from the map state at entry; handle -> list indices (the list holds duplicates and NULL entries)
        active = np.zeros((K, m), np.uint8)
        where = {}
        for i, h in enumerate(lst):
            h = int(h)
            if h < 0:
                continue
            where.setdefault(h, []).append(i)
            if map_ops.is_bad(h):
                continue
            for k in range(K):
                active[k, i] = not map_ops.in_target(h, k)
        best, idx, visible = (np.array(a) for a in candidates(list(targets), np.arange(m), desc, active))
        nFused = []
        for k in range(K):
            heirs = set()
            map_ops.begin_target(k)
            tail = _HeirLog(map_ops, where, heirs)
            n = (self.fuse_replay_sim3 if sim3 else self.fuse_replay)(lst, visible[k], best[k], idx[k], tail)
            map_ops.end_target(k, lambda i: heirs.update(where.get(int(lst[i]), ())))
            nFused.append(n)
            dirty = []
            for i in sorted(heirs):
                h = int(lst[i])
                if h < 0 or map_ops.is_bad(h):
                    continue
                d = np.frombuffer(bytes(map_ops.descriptor(h)), np.uint8)
                if not np.array_equal(d, desc[i]):
                    desc[i] = d
                    dirty.append(i)
            if dirty and k + 1 < K:
                dirty = np.array(dirty, np.int64)
                b, ix, vis = candidates(list(targets[k + 1:]), dirty, desc[dirty], active[k + 1:][:, dirty])
                best[k + 1:, dirty], idx[k + 1:, dirty], visible[k + 1:, dirty] = b, ix, vis
                stats["refreshes"] += 1
        ORBmatcher._last_fuse_keyframes = stats
        return nFused

    @staticmethod
    def distinctive_descriptors(desc, off):
        """MapPoint::ComputeDistinctiveDescriptors for a batch (MapPoint.cc:305-370)."""
        L = lib()
        d = np.ascontiguousarray(desc, np.uint8); o = np.ascontiguousarray(off, np.int32)
        best = np.zeros(len(o) - 1, np.int32)
        check(L.orbm_distinctive_descriptors(_p(d), _p(o), len(o) - 1, _p(best)))
        return best

    # ---------------------------------------------------------------- searches on a resident frame (orbm_frame)
    def frame_search_window(self, frame, queries, qdesc, skip=None, init_dist=256):
        q = np.ascontiguousarray(queries, self.WQ_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
        nq = len(q)
        outs = [np.zeros(nq, np.int32) for _ in range(5)]
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        check(self._L.orbm_frame_search_window(frame._h, _p(q), _p(qd), nq, _p(sk) if sk is not None else None, int(init_dist),
                                               *[_p(o) for o in outs]))
        return tuple(outs)

    def frame_search_fuse(self, frame, queries, qdesc, inv_level_sigma2=None):
        q = np.ascontiguousarray(queries, self.WQ_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
        sg = np.ascontiguousarray(inv_level_sigma2, np.float32) if inv_level_sigma2 is not None else None
        best = np.zeros(len(q), np.int32); idx = np.zeros(len(q), np.int32)
        check(self._L.orbm_frame_search_fuse(frame._h, _p(q), _p(qd), len(q), _p(sg) if sg is not None else None,
                                             len(sg) if sg is not None else 0, _p(best), _p(idx)))
        return best, idx

    def frame_search_projection(self, frame, queries, qdesc, qangle, qtakes, occupied=None, th_accept=None, ratio_same_level=False):
        """orbm_search_projection on a resident frame -> (match_kp, match_q, nmatches)."""
        asc = np.ascontiguousarray
        q = asc(queries, self.WQ_DTYPE); qd = asc(qdesc, np.uint8)
        qa = asc(qangle, np.float32) if qangle is not None else None     # (locals: a converted copy must outlive the call)
        qt = asc(qtakes, np.uint8) if qtakes is not None else None
        oc = asc(occupied, np.uint8) if occupied is not None else None
        nq = len(q)
        mk = np.zeros(max(frame.n, 1), np.int32); mq = np.zeros(nq, np.int32); nm = C.c_int(0)
        check(self._L.orbm_frame_search_projection(frame._h, _p(q), _p(qd), _p(qa) if qa is not None else None,
                                                   _p(qt) if qt is not None else None, nq, _p(oc) if oc is not None else None,
                                                   self.TH_HIGH if th_accept is None else int(th_accept), self.mfNNratio,
                                                   int(ratio_same_level), int(self.mbCheckOrientation), _p(mk), _p(mq), C.byref(nm)))
        return mk[:frame.n], mq, nm.value

    def frame_search_for_initialization(self, frame2, kps2, kps1, desc1, vbPrevMatched, windowSize=10):
        k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2); d1 = np.ascontiguousarray(desc1, np.uint8)
        pv = np.array(vbPrevMatched, np.float32, copy=True).reshape(-1, 2)
        m12 = np.zeros(len(k1), np.int32); nm = C.c_int(0)
        check(self._L.orbm_frame_search_for_initialization(frame2._h, _p(k2), _p(k1), _p(d1), len(k1), _p(pv), int(windowSize),
                                                           self.mfNNratio, int(self.mbCheckOrientation), _p(m12), C.byref(nm)))
        return m12, pv, nm.value

    def frame_search_by_projection_map(self, frame, has_mp, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, Rcw, tcw, cam,
                                       scale_factors, th=1.0):
        hm = np.ascontiguousarray(has_mp, np.uint8)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos), f32(mp_normal), f32(mp_min_dist), f32(mp_max_dist)
        md = np.ascontiguousarray(mp_desc, np.uint8)
        R = np.ascontiguousarray(Rcw, np.float64).reshape(9); t = np.ascontiguousarray(tcw, np.float64).reshape(3)
        cam = np.ascontiguousarray(cam, self.CAM_DTYPE).reshape(1)
        sc = f32(scale_factors)
        m = len(pos)
        matched = np.zeros(max(frame.n, 1), np.int32); proj = np.zeros((m, 4), np.float32); nm = C.c_int(0)
        check(self._L.orbm_frame_search_by_projection_map(frame._h, _p(hm), _p(pos), _p(nrm), _p(mn), _p(mx), _p(md), m, _p(R), _p(t),
                                                          _p(cam), _p(sc), len(sc), th, self.mfNNratio, self.TH_RELOC,
                                                          _p(matched), C.byref(nm), _p(proj)))
        return matched[:frame.n], nm.value, proj

    # ---------------------------------------------------------------- the whole-map search under P poses in one call
    def SearchByProjectionMapPoses(self, kps, desc, has_mp, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc, Rcw, tcw, cam,
                                   scale_factors, th=1.0, want_proj=True):
        """SearchByProjection(Frame&, Map*, Rcw, tcw, ...) (ORBmatcher.cc:134-222) under P poses in one launch
        (orbm_search_by_projection_map_poses): Rcw[P, 3, 3], tcw[P, 3]; frame and map travel with the call.
        Returns (vMatchedMPs[P, n] as indices or -1, nmatches[P], proj[P, m, 4] or None): row p = SearchByProjectionMap at pose p."""
        kps = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
        hm = np.ascontiguousarray(has_mp, np.uint8) if has_mp is not None else None
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos), f32(mp_normal), f32(mp_min_dist), f32(mp_max_dist)
        md = np.ascontiguousarray(mp_desc, np.uint8)
        R, t, P = _poses(Rcw, tcw)
        cam = np.ascontiguousarray(cam, self.CAM_DTYPE).reshape(1)
        sc = f32(scale_factors)
        n, m = len(kps), len(pos)
        matched = np.zeros((P, n), np.int32); nm = np.zeros(P, np.int32)
        proj = np.zeros((P, m, 4), np.float32) if want_proj else None
        check(self._L.orbm_search_by_projection_map_poses(_p(kps), _p(d), n, _p(hm) if hm is not None else None, _p(pos), _p(nrm), _p(mn),
                                                          _p(mx), _p(md), m, _p(R), _p(t), P, _p(cam), _p(sc), len(sc), th, self.mfNNratio,
                                                          self.TH_RELOC, _p(matched), _p(nm), _p(proj) if want_proj else None))
        return matched, nm, proj

    def frame_search_by_projection_map_poses(self, frame, has_mp, snapshot, Rcw, tcw, cam, scale_factors, th=1.0, want_proj=True):
        """The same on a resident frame and a MapSnapshot (orbm_frame_search_by_projection_map_poses): the call uploads
        has_mp, the poses and the scale factors only."""
        hm = np.ascontiguousarray(has_mp, np.uint8) if has_mp is not None else None
        R, t, P = _poses(Rcw, tcw)
        cam = np.ascontiguousarray(cam, self.CAM_DTYPE).reshape(1)
        sc = np.ascontiguousarray(scale_factors, np.float32)
        n, m = frame.n, snapshot.m
        matched = np.zeros((P, n), np.int32); nm = np.zeros(P, np.int32)
        proj = np.zeros((P, m, 4), np.float32) if want_proj else None
        check(self._L.orbm_frame_search_by_projection_map_poses(frame._h, _p(hm) if hm is not None else None, snapshot._h, _p(R), _p(t), P,
                                                                _p(cam), _p(sc), len(sc), th, self.mfNNratio, self.TH_RELOC, _p(matched),
                                                                _p(nm), _p(proj) if want_proj else None))
        return matched, nm, proj

    @staticmethod
    def last_map_poses_waits():
        """orbm_debug_last_map_poses_waits: host waits of the last ..._map_poses call of this process (1 when it launched)."""
        return lib().orbm_debug_last_map_poses_waits()

    def frame_search_by_bow(self, frame1, fv1, valid1, frame2, fv2, valid2=None, kf_kf=False):
        """SearchByBoW on two resident frames (orbm_frame_search_by_bow): fv = feature_vector_arrays(...) of each side.
        Returns (match12, match21, nmatches)."""
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        nodes1, off1, it1 = [i32(a) for a in fv1]; nodes2, off2, it2 = [i32(a) for a in fv2]
        v1 = np.ascontiguousarray(valid1, np.uint8)
        v2 = np.ascontiguousarray(valid2, np.uint8) if kf_kf else None
        m12 = np.zeros(max(frame1.n, 1), np.int32); m21 = np.zeros(max(frame2.n, 1), np.int32); nm = C.c_int(0)
        check(self._L.orbm_frame_search_by_bow(frame1._h, _p(nodes1), _p(off1), _p(it1), len(nodes1), _p(v1), frame2._h, _p(nodes2),
                                               _p(off2), _p(it2), len(nodes2), _p(v2) if v2 is not None else None, self.TH_LOW, int(kf_kf),
                                               self.mfNNratio, int(self.mbCheckOrientation), _p(m12), _p(m21), C.byref(nm)))
        return m12[:frame1.n], m21[:frame2.n], nm.value

    MAX_BOW_PAIRS = 64

    def frame_search_by_bow_pairs(self, pairs, kf_kf=False):
        """K searches of frame_search_by_bow in one call (orbm_frame_search_by_bow_pairs): pairs = a sequence of
        (frame1, fv1, valid1, frame2, fv2, valid2), each as that method takes them (valid2 is used only with kf_kf); a frame may
        stand in any number of pairs.  Returns a list of (match12, match21, nmatches), one per pair: what the single call gives."""
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        K = len(pairs)
        arr = (_CBowPair * max(K, 1))()
        keep, rows = [], []
        for c, (frame1, fv1, valid1, frame2, fv2, valid2) in zip(arr, pairs):
            nodes1, off1, it1 = [i32(a) for a in fv1]; nodes2, off2, it2 = [i32(a) for a in fv2]
            v1 = np.ascontiguousarray(valid1, np.uint8)
            v2 = np.ascontiguousarray(valid2, np.uint8) if kf_kf else None
            m12 = np.zeros(max(frame1.n, 1), np.int32); m21 = np.zeros(max(frame2.n, 1), np.int32)
            keep.append((nodes1, off1, it1, v1, nodes2, off2, it2, v2))
            rows.append((m12[:frame1.n], m21[:frame2.n]))
            a = lambda x: _p(x).value if x is not None else None
            h = lambda f: f._h.value if isinstance(f._h, C.c_void_p) else f._h
            c.frame1, c.nodes1, c.off1, c.items1, c.nn1, c.valid1 = h(frame1), a(nodes1), a(off1), a(it1), len(nodes1), a(v1)
            c.frame2, c.nodes2, c.off2, c.items2, c.nn2, c.valid2 = h(frame2), a(nodes2), a(off2), a(it2), len(nodes2), a(v2)
            c.match12, c.match21 = a(m12), a(m21)
        nm = np.zeros(max(K, 1), np.int32)
        check(self._L.orbm_frame_search_by_bow_pairs(arr if K else None, K, self.TH_LOW, int(kf_kf), self.mfNNratio,
                                                     int(self.mbCheckOrientation), _p(nm)))
        return [(m12, m21, int(nm[k])) for k, (m12, m21) in enumerate(rows)]

    @staticmethod
    def last_bow_pairs_waits():
        """orbm_debug_last_bow_pairs_waits: host waits of the last frame_search_by_bow_pairs call of this process (0: no pair had a
        query; 1 on the common path; one more per pair repeated on the sequential resolver)."""
        return lib().orbm_debug_last_bow_pairs_waits()

    def frame_search_for_triangulation(self, kf1, fv1, has_mp1, kf2, fv2, has_mp2, F12, ex, ey, scale_factors2, level_sigma2,
                                       bOnlyStereo=False):
        """SearchForTriangulation on two resident keyframes (orbm_frame_search_for_triangulation).
        Returns (vMatchedPairs as an (m, 2) array, nmatches, vMatches12)."""
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        (nd1, of1, it1), (nd2, of2, it2) = (tuple(i32(a) for a in fv) for fv in (fv1, fv2))
        h1 = np.ascontiguousarray(has_mp1, np.uint8); h2 = np.ascontiguousarray(has_mp2, np.uint8)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sf = np.ascontiguousarray(scale_factors2, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
        m12 = np.full(max(kf1.n, 1), -1, np.int32); nm = C.c_int(0)
        check(self._L.orbm_frame_search_for_triangulation(kf1._h, _p(nd1), _p(of1), _p(it1), len(nd1), _p(h1), kf2._h, _p(nd2), _p(of2),
                                                          _p(it2), len(nd2), _p(h2), int(bool(bOnlyStereo)), _p(F), float(ex), float(ey),
                                                          _p(sf), _p(sg), len(sf), int(self.mbCheckOrientation), _p(m12), C.byref(nm)))
        m12 = m12[:kf1.n]
        i1 = np.nonzero(m12 >= 0)[0]
        return np.stack([i1, m12[i1]], 1), nm.value, m12

    # ---------------------------------------------------------------- the projection searches as whole functions
    def SearchByProjectionLast(self, cur, view, Tcw, Tlw, last, occupied, th, bMono, want_queries=False):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1529-1671) in one call: cur = resident
        current frame, view = View(...), last = Points(valid, pos, desc, takes, octave, angle) per keypoint of the last frame,
        occupied[j] = mvpMapPoints[j] holds an observed point.  Returns (match_kp, match_q, nmatches[, queries])."""
        return self._whole(self._L.orbm_search_by_projection_last, cur, view, [Tcw, Tlw], last, occupied,
                           [th, int(bool(bMono)), self.TH_HIGH, int(self.mbCheckOrientation)], want_queries)

    def SearchByProjectionPoints(self, cur, view, Tcw, points, occupied, th=1.0, viewing_cos_limit=0.5):
        """Tracking::SearchLocalPoints' data plane: Frame::isInFrustum for every listed point chained into
        SearchByProjection(Frame&, vector<MapPoint*>&, th) (ORBmatcher.cc:46-132) on a resident frame.
        Returns (match_kp, match_q, nmatches, projected[PROJ_DTYPE], queries)."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        oc = np.ascontiguousarray(occupied, np.uint8) if occupied is not None else None
        mk = np.zeros(max(cur.n, 1), np.int32); mq = np.zeros(max(points.n, 1), np.int32); nm = C.c_int(0)
        proj = np.zeros(max(points.n, 1), self.PROJ_DTYPE); q = np.zeros(max(points.n, 1), self.WQ_DTYPE)
        check(self._L.orbm_search_by_projection_points(cur._h, C.byref(view.c), _p(T), C.byref(points.c),
                                                       _p(oc) if oc is not None else None, th, viewing_cos_limit, self.TH_HIGH,
                                                       self.mfNNratio, _p(mk), _p(mq), C.byref(nm), _p(proj), _p(q)))
        return mk[:cur.n], mq[:points.n], nm.value, proj[:points.n], q[:points.n]

    def SearchByProjectionKeyFrame(self, cur, view, Tcw, kf, occupied, th, ORBdist, want_queries=False):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1673-1800)."""
        return self._whole(self._L.orbm_search_by_projection_keyframe, cur, view, [Tcw], kf, occupied,
                           [th, int(ORBdist), int(self.mbCheckOrientation)], want_queries)

    def SearchByProjectionSim3(self, kf, view, Scw, points, occupied, th, want_queries=False):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:491-604)."""
        return self._whole(self._L.orbm_search_by_projection_sim3, kf, view, [Scw], points, occupied, [int(th), self.TH_LOW], want_queries)

    def _whole(self, fn, frame, view, poses, pts, occupied, scalars, want_queries):
        mats = [np.ascontiguousarray(T, np.float32).reshape(16) for T in poses]
        oc = np.ascontiguousarray(occupied, np.uint8) if occupied is not None else None
        mk = np.zeros(max(frame.n, 1), np.int32); mq = np.zeros(max(pts.n, 1), np.int32); nm = C.c_int(0)
        q = np.zeros(max(pts.n, 1), self.WQ_DTYPE) if want_queries else None
        check(fn(frame._h, C.byref(view.c), *[_p(m) for m in mats], C.byref(pts.c), _p(oc) if oc is not None else None, *scalars,
                 _p(mk), _p(mq), C.byref(nm), _p(q) if q is not None else None))
        out = (mk[:frame.n], mq[:pts.n], nm.value)
        return out + (q[:pts.n],) if want_queries else out

    # ---------------------------------------------------------------- a frame tracked in one call
    def TrackWithMotionModel(self, cur, view, cam, inv_level_sigma2, Tcw, Tlw, last, th, bMono, min_matches=20, outlier_fill=0):
        """Tracking::TrackWithMotionModel (Tracking.cc:1232-1284, behind UpdateLastFrame) in one call (orbm_track_with_motion_model):
        SearchByProjection(Cur, Last, th, bMono), again with 2 * th below min_matches, PoseOptimization from Tcw over the matches
        and the counts of the discard loop.  cam = (fx, fy, cx, cy, mbf), inv_level_sigma2 = mvInvLevelSigma2 (the pose solve's);
        Tcw = the predicted pose.  outlier_fill presets the outlier array (written only where match_kp >= 0).
        Returns (TrackResult, match_kp, match_q, outlier, Tcw_out float32[4, 4], PoseStats)."""
        from .pose import PoseStats, _camera
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16); Tl = np.ascontiguousarray(Tlw, np.float32).reshape(16)
        mk = np.zeros(max(cur.n, 1), np.int32); mq = np.zeros(max(last.n, 1), np.int32)
        out = np.full(max(cur.n, 1), outlier_fill, np.uint8); Tout = np.zeros(16, np.float32)
        res = TrackResult(); st = PoseStats(); c = _camera(cam, inv_level_sigma2)
        check(self._L.orbm_track_with_motion_model(cur._h, C.byref(view.c), C.byref(c), _p(T), _p(Tl), C.byref(last.c), th, int(bool(bMono)),
                                                   self.TH_HIGH, int(self.mbCheckOrientation), int(min_matches), _p(mk), _p(mq), _p(out),
                                                   _p(Tout), C.byref(res), C.byref(st)))
        return res, mk[:cur.n], mq[:last.n], out[:cur.n], Tout.reshape(4, 4), st

    def TrackLocalMap(self, cur, view, cam, inv_level_sigma2, Tcw, points, base_has, base_pos, base_takes, th=1.0, viewing_cos_limit=0.5,
                      outlier_fill=0):
        """Tracking::TrackLocalMap (Tracking.cc:1294-1320, behind UpdateLocalMap) in one call (orbm_track_local_map): isInFrustum +
        SearchByProjection(F, vpMapPoints, th), PoseOptimization over the union of the new matches and the slots the frame holds
        (base_has[n], base_pos[n, 3], base_takes[n]; base_has None: none) and the counts of the statistics loop.
        Returns (TrackResult, match_kp, match_q, projected[PROJ_DTYPE], outlier, Tcw_out float32[4, 4], PoseStats)."""
        from .pose import PoseStats, _camera
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        bh = np.ascontiguousarray(base_has, np.uint8) if base_has is not None else None
        bp = np.ascontiguousarray(base_pos, np.float32) if base_has is not None else None
        bt = np.ascontiguousarray(base_takes, np.uint8) if base_has is not None and base_takes is not None else None
        mk = np.zeros(max(cur.n, 1), np.int32); mq = np.zeros(max(points.n, 1), np.int32)
        proj = np.zeros(max(points.n, 1), self.PROJ_DTYPE)
        out = np.full(max(cur.n, 1), outlier_fill, np.uint8); Tout = np.zeros(16, np.float32)
        res = TrackResult(); st = PoseStats(); c = _camera(cam, inv_level_sigma2)
        opt = lambda a: _p(a) if a is not None else None
        check(self._L.orbm_track_local_map(cur._h, C.byref(view.c), C.byref(c), _p(T), C.byref(points.c), opt(bh), opt(bp), opt(bt), th,
                                           viewing_cos_limit, self.TH_HIGH, self.mfNNratio, _p(mk), _p(mq), _p(proj), _p(out), _p(Tout),
                                           C.byref(res), C.byref(st)))
        return res, mk[:cur.n], mq[:points.n], proj[:points.n], out[:cur.n], Tout.reshape(4, 4), st

    @staticmethod
    def last_track_waits():
        """orbm_debug_last_track_waits: host waits of the last Track* call of this process (1 on the common path)."""
        return lib().orbm_debug_last_track_waits()

    # ---------------------------------------------------------------- LocalMapping::CreateNewMapPoints in one call
    TRI_NO_MATCH, TRI_CREATED, TRI_SKIPPED, TRI_SVD_ZERO, TRI_PARALLAX, TRI_DEPTH, TRI_REPROJ1, TRI_REPROJ2, TRI_DIST_ZERO, TRI_SCALE = range(-1, 9)
    TRI_NSTATUS = 9

    @staticmethod
    def CreateNewMapPoints(cur, neighbours, scale_factors, level_sigma2, scale_factor):
        """LocalMapping::CreateNewMapPoints' loop over the neighbour keyframes (LocalMapping.cc:281-517) in one call
        (orbm_create_new_map_points): cur / neighbours = TriangKeyFrame, the neighbours in the reference's order, each with its
        F12 and epipole.  Returns a CreatedPoints: match12[K, n1], status[K, n1] (TRI_*), x3d[K, n1, 3] (NaN where nothing was
        created), counts[K, TRI_NSTATUS], nnew, and created() = the creation list in the reference's order."""
        sf = np.ascontiguousarray(scale_factors, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
        if len(sf) != len(sg):
            raise ValueError("scale_factors and level_sigma2 differ in length")
        K, n1 = len(neighbours), cur.n
        arr = (_CTriangKeyFrame * max(K, 1))(*[nb.c for nb in neighbours])
        m12 = np.full((K, n1), -1, np.int32); st = np.full((K, n1), -1, np.int8); x3d = np.full((K, n1, 3), np.nan, np.float32)
        counts = np.zeros((K, ORBmatcher.TRI_NSTATUS), np.int32); nnew = C.c_int(0)
        check(lib().orbm_create_new_map_points(C.byref(cur.c), arr if K else None, K, _p(sf), _p(sg), len(sf), float(scale_factor),
                                               _p(m12), _p(st), _p(x3d), _p(counts), C.byref(nnew)))
        return CreatedPoints(m12, st, x3d, counts, nnew.value)

    @staticmethod
    def last_create_points_waits():
        """orbm_debug_last_create_points_waits: host waits of the last CreateNewMapPoints call of this process."""
        return lib().orbm_debug_last_create_points_waits()

    def SearchBySim3Whole(self, kf1, kf2, view, T1w, T2w, s12, R12, t12, points1, points2, th, want_queries=False):
        """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1303-1527) in one call.  Returns (match12, nFound, vnMatch1, vnMatch2[, q12, q21])."""
        f32 = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(k)
        T1, T2, R, t = f32(T1w, 16), f32(T2w, 16), f32(R12, 9), f32(t12, 3)
        n1, n2 = kf1.n, kf2.n
        v1 = np.zeros(max(n1, 1), np.int32); v2 = np.zeros(max(n2, 1), np.int32); m12 = np.zeros(max(n1, 1), np.int32); nf = C.c_int(0)
        q12 = np.zeros(max(n1, 1), self.WQ_DTYPE) if want_queries else None; q21 = np.zeros(max(n2, 1), self.WQ_DTYPE) if want_queries else None
        check(self._L.orbm_search_by_sim3(kf1._h, kf2._h, C.byref(view.c), _p(T1), _p(T2), s12, _p(R), _p(t), C.byref(points1.c),
                                          C.byref(points2.c), th, self.TH_HIGH, _p(v1), _p(v2), _p(m12), C.byref(nf),
                                          _p(q12) if want_queries else None, _p(q21) if want_queries else None))
        out = (m12[:n1], nf.value, v1[:n1], v2[:n2])
        return out + (q12[:n1], q21[:n2]) if want_queries else out


def _poses(Rcw, tcw):
    """Rcw[P, 3, 3] (or [P, 9]), tcw[P, 3] as the flat double arrays of the ..._map_poses entries."""
    R = np.ascontiguousarray(Rcw, np.float64).reshape(-1, 9); t = np.ascontiguousarray(tcw, np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError("Rcw and tcw differ in the number of poses")
    return R, t, len(R)


class TrackResult(C.Structure):
    """orbm_track_result"""
    _fields_ = [("tracked", C.c_int32), ("search_used", C.c_int32), ("nsearch", C.c_int32), ("ngood", C.c_int32), ("nmatches", C.c_int32),
                ("nmatches_map", C.c_int32)]


class _CPoints(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p),
                ("max_distance", C.c_void_p), ("desc", C.c_void_p), ("takes", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p)]


class _CView(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float),
                ("log_scale_factor", C.c_float), ("nlevels", C.c_int32), ("scale_factors", C.c_void_p)]


class _HeirLog:
    """map_ops as the Fuse tails see it, noting every list index whose handle a replace(dead, heir) names as the heir."""

    def __init__(self, map_ops, where, heirs):
        self._ops, self._where, self._heirs = map_ops, where, heirs

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def replace(self, dead, heir):
        self._ops.replace(dead, heir)
        self._heirs.update(self._where.get(int(heir), ()))


class _CCamera(C.Structure):
    """orbm_camera (ORBmatcher.CAM_DTYPE as a ctypes structure)"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("min_x", C.c_int32), ("max_x", C.c_int32),
                ("min_y", C.c_int32), ("max_y", C.c_int32), ("grid_min_x", C.c_float), ("grid_min_y", C.c_float), ("grid_max_x", C.c_float),
                ("grid_max_y", C.c_float)]


class _CFuseTarget(C.Structure):
    """orbm_fuse_target"""
    _fields_ = [("frame", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("cam", _CCamera),
                ("mbf", C.c_float)]


class FuseTarget:
    """orbm_fuse_target: a resident keyframe with the pose and camera ORBmatcher::Fuse projects with.  Rcw, tcw, Ow as
    project_points takes them (Sim3 form: sRcw / s, t / s, -Rcw' tcw, ORBmatcher.cc:1188-1192); cam = one CAM_DTYPE record."""

    def __init__(self, frame, Rcw, tcw, Ow, cam, mbf):
        f32 = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
        self.frame = frame
        self.Rcw, self.tcw, self.Ow, self.mbf = f32(Rcw, 9), f32(tcw, 3), f32(Ow, 3), float(mbf)
        self.cam = np.ascontiguousarray(cam, ORBmatcher.CAM_DTYPE).reshape(1).copy()
        h = frame._h if frame is not None else None
        self.c = _CFuseTarget(h.value if isinstance(h, C.c_void_p) else h, (C.c_float * 9)(*self.Rcw.tolist()), (C.c_float * 3)(*self.tcw.tolist()),
                              (C.c_float * 3)(*self.Ow.tolist()), _CCamera.from_buffer_copy(self.cam.tobytes()), self.mbf)


class _CBowPair(C.Structure):
    """orbm_bow_pair"""
    _fields_ = [("frame1", C.c_void_p), ("nodes1", C.c_void_p), ("off1", C.c_void_p), ("items1", C.c_void_p), ("nn1", C.c_int32),
                ("valid1", C.c_void_p), ("frame2", C.c_void_p), ("nodes2", C.c_void_p), ("off2", C.c_void_p), ("items2", C.c_void_p),
                ("nn2", C.c_int32), ("valid2", C.c_void_p), ("match12", C.c_void_p), ("match21", C.c_void_p)]


class _CTriangKeyFrame(C.Structure):
    """orbm_triang_keyframe"""
    _fields_ = [("frame", C.c_void_p), ("Tcw", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("invfx", C.c_float), ("invfy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float), ("depth", C.c_void_p),
                ("has_mappoint", C.c_void_p), ("nodes", C.c_void_p), ("off", C.c_void_p), ("items", C.c_void_p), ("nn", C.c_int32),
                ("F12", C.c_void_p), ("ex", C.c_float), ("ey", C.c_float)]


class TriangKeyFrame:
    """orbm_triang_keyframe: a resident keyframe with what CreateNewMapPoints reads of it.  cam = (fx, fy, cx, cy, mb, mbf)
    (invfx = 1 / fx in float, as KeyFrame holds it); fv = feature_vector_arrays(...); depth = mvDepth, or None if no keypoint
    of the frame is stereo; F12 / ex / ey: for a neighbour."""

    def __init__(self, frame, Tcw, cam, fv, has_mappoint, depth=None, F12=None, ex=0.0, ey=0.0):
        f32 = lambda a: np.ascontiguousarray(a, np.float32) if a is not None else None
        fx, fy, cx, cy, mb, mbf = (np.float32(v) for v in cam)
        nodes, off, items = (np.ascontiguousarray(a, np.int32) for a in fv)
        self.frame, self.n = frame, frame.n
        self._keep = dict(Tcw=f32(Tcw).reshape(16), depth=f32(depth), has=np.ascontiguousarray(has_mappoint, np.uint8), nodes=nodes, off=off,
                          items=items, F12=f32(F12).reshape(9) if F12 is not None else None)
        k = self._keep
        opt = lambda a: _p(a) if a is not None else None
        self.c = _CTriangKeyFrame(frame._h, _p(k["Tcw"]), fx, fy, cx, cy, np.float32(1) / fx, np.float32(1) / fy, mb, mbf, opt(k["depth"]),
                                  _p(k["has"]), _p(nodes), _p(off), _p(items), len(nodes), opt(k["F12"]), float(ex), float(ey))


class CreatedPoints:
    """Results of ORBmatcher.CreateNewMapPoints."""

    def __init__(self, match12, status, x3d, counts, nnew):
        self.match12, self.status, self.x3d, self.counts, self.nnew = match12, status, x3d, counts, nnew

    def created(self):
        """(k, idx1, idx2, x3D[3]) arrays of the created points, (k, idx1) ascending: the reference's creation order."""
        k, i = np.nonzero(self.status == ORBmatcher.TRI_CREATED)
        return k, i, self.match12[k, i], self.x3d[k, i]


class Points:
    """orbm_points: the flat form of a vector<MapPoint*> (see include/orbslam_hip.h)."""

    def __init__(self, valid, pos, desc, normal=None, min_distance=None, max_distance=None, takes=None, octave=None, angle=None):
        f32 = lambda a: np.ascontiguousarray(a, np.float32) if a is not None else None
        u8 = lambda a: np.ascontiguousarray(a, np.uint8) if a is not None else None
        self._keep = dict(valid=u8(valid), pos=f32(pos), normal=f32(normal), min_distance=f32(min_distance),
                          max_distance=f32(max_distance), desc=u8(desc), takes=u8(takes),
                          octave=np.ascontiguousarray(octave, np.int32) if octave is not None else None, angle=f32(angle))
        self.n = len(self._keep["valid"])
        self.c = _CPoints(self.n, *[(_p(self._keep[k]) if self._keep[k] is not None else None)
                                    for k in ("valid", "pos", "normal", "min_distance", "max_distance", "desc", "takes", "octave", "angle")])


class View:
    """orbm_view: calibration and scale pyramid of the searched frame."""

    def __init__(self, fx, fy, cx, cy, mb, mbf, log_scale_factor, scale_factors):
        self._sc = np.ascontiguousarray(scale_factors, np.float32)
        self.c = _CView(fx, fy, cx, cy, mb, mbf, log_scale_factor, len(self._sc), _p(self._sc))


class Distortion(C.Structure):
    """orbm_distortion: mK (fx, fy, cx, cy) and mDistCoef (k1, k2, p1, p2, k3) of a launch file.  k1 == 0: no undistortion."""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        super().__init__(fx, fy, cx, cy, k1, k2, p1, p2, k3)


def image_bounds(camera, width, height):
    """Frame::ComputeImageBounds: (mnMinX, mnMinY, mnMaxX, mnMaxY) as float32 (host only)."""
    b = np.zeros(4, np.float32)
    check(lib().orbm_image_bounds(C.byref(camera), int(width), int(height), _p(b)))
    return tuple(b)


def undistort_points(camera, xy):
    """Frame::UndistortKeyPoints on an (n, 2) float32 array, on the device."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(xy)
    check(lib().orbm_undistort_points(C.byref(camera), _p(xy) if len(xy) else None, len(xy), _p(out) if len(xy) else None))
    return out


class Frame:
    """orbm_frame: a Frame / KeyFrame resident in HBM (grid built once, on the device)."""

    def __init__(self, kps=None, desc=None, bounds=(0.0, 0.0, 640.0, 480.0), uright=None, _handle=None):
        self._L = lib()
        self._h = C.c_void_p()
        self.bounds = tuple(float(b) for b in bounds)
        if _handle is not None:
            self._h = _handle
        else:
            k = np.ascontiguousarray(kps); d = np.ascontiguousarray(desc, np.uint8)
            ur = np.ascontiguousarray(uright, np.float32) if uright is not None else None
            check(self._L.orbm_frame_create(_p(k), _p(d), len(k), _p(ur) if ur is not None else None, *self.bounds, C.byref(self._h)))
        n = C.c_int(0); ns = C.c_int(0)
        check(self._L.orbm_frame_size(self._h, C.byref(n), C.byref(ns)))
        self.n, self.ns = n.value, ns.value

    @classmethod
    def from_extractor(cls, ex, frame=0, bounds=(0.0, 0.0, 640.0, 480.0), xy_undistorted=None, uright=None, uright_from_stereo=False,
                       camera=None):
        """camera (a Distortion): Frame::UndistortKeyPoints runs inside the frame build (orbm_frame_from_extractor_cam); it and
        xy_undistorted exclude each other."""
        L = lib()
        h = C.c_void_p()
        xy = np.ascontiguousarray(xy_undistorted, np.float32) if xy_undistorted is not None else None
        ur = np.ascontiguousarray(uright, np.float32) if uright is not None else None
        if camera is not None:
            if xy is not None:
                raise ValueError("camera and xy_undistorted exclude each other")
            check(L.orbm_frame_from_extractor_cam(ex._h, int(frame), C.byref(camera), _p(ur) if ur is not None else None,
                                                  int(bool(uright_from_stereo)), *[float(b) for b in bounds], C.byref(h)))
        else:
            check(L.orbm_frame_from_extractor(ex._h, int(frame), _p(xy) if xy is not None else None, _p(ur) if ur is not None else None,
                                              int(bool(uright_from_stereo)), *[float(b) for b in bounds], C.byref(h)))
        return cls(bounds=bounds, _handle=h)

    @classmethod
    def batch_from_extractor(cls, ex, first, count, bounds=(0.0, 0.0, 640.0, 480.0), camera=None, uright_from_stereo=False):
        """orbm_frames_from_extractor: frames first .. first + count - 1 of the extractor's last batch in ONE launch; a list of Frames."""
        hs = (C.c_void_p * max(int(count), 1))()
        check(lib().orbm_frames_from_extractor(ex._h, int(first), int(count), C.byref(camera) if camera is not None else None,
                                               int(bool(uright_from_stereo)), *[float(b) for b in bounds], hs))
        return [cls(bounds=bounds, _handle=C.c_void_p(hs[i])) for i in range(int(count))]

    @staticmethod
    def last_build_waits():
        """orbm_debug_last_frame_build_waits: host waits of the last frame-making call of this process."""
        return lib().orbm_debug_last_frame_build_waits()

    def keypoints_un(self):
        """orbm_frame_keypoints_un: the mvKeysUn coordinates by keypoint index, (n, 2) float32 (what the searches use)."""
        xy = np.zeros((self.n, 2), np.float32)
        check(self._L.orbm_frame_keypoints_un(self._h, _p(xy) if self.n else None))
        return xy

    def alias(self, bounds):
        """orbm_frame_alias: the same device data searched with other bounds (a KeyFrame's int-valued mnMinX .. mnMaxY)."""
        h = C.c_void_p()
        check(self._L.orbm_frame_alias(self._h, *[float(b) for b in bounds], C.byref(h)))
        return Frame(bounds=bounds, _handle=h)

    def layout(self):
        perm = np.zeros(max(self.ns, 1), np.int32); cell_off = np.zeros(64 * 48 + 1, np.int32)
        check(self._L.orbm_frame_layout(self._h, _p(perm), _p(cell_off)))
        return perm[:self.ns], cell_off

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbm_frame_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class MapSnapshot:
    """orbm_map: what pMap->GetAllMapPoints() returned, flat and resident in HBM (immutable; made once per relocalisation).
    mp_min_dist / mp_max_dist are the GetMinDistanceInvariance() / GetMaxDistanceInvariance() values."""

    def __init__(self, mp_pos, mp_normal, mp_min_dist, mp_max_dist, mp_desc):
        self._L = lib()
        self._h = C.c_void_p()
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, nrm, mn, mx = f32(mp_pos).reshape(-1, 3), f32(mp_normal).reshape(-1, 3), f32(mp_min_dist), f32(mp_max_dist)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        if not (len(pos) == len(nrm) == len(mn) == len(mx) == len(md)):
            raise ValueError("the map arrays differ in length")
        check(self._L.orbm_map_create(_p(pos), _p(nrm), _p(mn), _p(mx), _p(md), len(pos), C.byref(self._h)))
        m = C.c_int(0)
        check(self._L.orbm_map_size(self._h, C.byref(m)))
        self.m = m.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbm_map_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
