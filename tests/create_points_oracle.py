"""ctypes wrapper of tests/create_points_oracle.c, the CPU restatement of the per-pair arithmetic of
LocalMapping::CreateNewMapPoints, and the loop over the neighbours around it and the oracle's literal SearchForTriangulation
(test infrastructure: never part of the product).  The C file is compiled on first use into a per-user cache directory
(tests/c_oracle.py).

No OpenCV exists for this project to run, so the restated cv::SVD (JacobiSVDImpl_<float>) is unpinned like the other OpenCV
primitives; tests/test_cpu_create_points.py checks it from first principles against numpy in float64."""
import ctypes as C
import os

import numpy as np

import c_oracle
import oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "create_points_oracle.c")
_LIB = None

STATUS = dict(NO_MATCH=-1, CREATED=0, SKIPPED=1, SVD_ZERO=2, PARALLAX=3, DEPTH=4, REPROJ1=5, REPROJ2=6, DIST_ZERO=7, SCALE=8)
NSTATUS = 9

CAM_DTYPE = np.dtype([("Tcw", "f4", 16), ("fx", "f4"), ("fy", "f4"), ("cx", "f4"), ("cy", "f4"), ("invfx", "f4"), ("invfy", "f4"),
                      ("mb", "f4"), ("mbf", "f4")])                                                   # cpo_cam
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("uright", "f4"), ("depth", "f4"), ("octave", "i4")])   # cpo_kp
RESULT_DTYPE = np.dtype([("status", "i4"), ("from_svd", "i4"), ("sweeps", "i4"), ("x3d", "f4", 3), ("A", "f4", 16), ("gap", "f8")],
                        align=True)                                                                    # cpo_result


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(c_oracle.build(_SRC))
        vp = C.c_void_p
        L.cpo_pairs.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_float, vp]
        L.cpo_pairs.restype = None
        L.cpo_svd_vt3.argtypes = [vp, vp]
        L.cpo_svd_vt3.restype = C.c_int
        L.cpo_pose_parts.argtypes = [vp] * 5
        L.cpo_pose_parts.restype = None
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def svd_vt3(A):
    """vt.row(3) of the restated cv::SVD::compute of a 4 x 4 float matrix, and the number of sweeps"""
    A = np.ascontiguousarray(A, np.float32).reshape(16); v = np.zeros(4, np.float32)
    return v, lib().cpo_svd_vt3(_p(A), _p(v))


def cam_of(kf):
    c = np.zeros(1, CAM_DTYPE)
    fx, fy, cx, cy, mb, mbf = (np.float32(v) for v in kf["cam"])
    c["Tcw"][0] = np.asarray(kf["Tcw"], np.float32).reshape(16)
    c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"] = fx, fy, cx, cy, mb, mbf
    c["invfx"], c["invfy"] = np.float32(1) / fx, np.float32(1) / fy
    return c


def kps_of(kf):
    k = np.zeros(kf["n"], KP_DTYPE)
    k["x"], k["y"], k["octave"] = kf["kps"]["x"], kf["kps"]["y"], kf["kps"]["octave"]
    k["uright"] = -1.0 if kf["uright"] is None else kf["uright"]
    k["depth"] = -1.0 if kf["depth"] is None else kf["depth"]
    return k


def triangulate_pairs(scene, k, idx1, idx2):
    """cpo_result of the pairs (idx1[p] of the current keyframe, idx2[p] of neighbour k)"""
    cur, nb = scene["cur"], scene["neigh"][k]
    i1 = np.ascontiguousarray(idx1, np.int32); i2 = np.ascontiguousarray(idx2, np.int32)
    out = np.zeros(len(i1), RESULT_DTYPE)
    c1, c2, k1, k2 = cam_of(cur), cam_of(nb), kps_of(cur), kps_of(nb)
    sf = np.ascontiguousarray(scene["sf"], np.float32); sg = np.ascontiguousarray(scene["sg"], np.float32)
    lib().cpo_pairs(_p(c1), _p(c2), _p(k1), _p(k2), _p(i1), _p(i2), len(i1), _p(sf), _p(sg), float(scene["scale_factor"]), _p(out))
    return out


def search(scene, k, has1):
    """SearchForTriangulation(cur, neighbour k, F12, .., false) of a matcher without the orientation check (LocalMapping.cc:259, :315)"""
    cur, nb = scene["cur"], scene["neigh"][k]
    s1 = np.zeros(cur["n"], bool) if cur["uright"] is None else cur["uright"] >= 0
    s2 = np.zeros(nb["n"], bool) if nb["uright"] is None else nb["uright"] >= 0
    if cur["n"] == 0 or nb["n"] == 0:
        return np.full(cur["n"], -1, np.int32)
    return oracle.search_for_triangulation(cur["kps"], cur["desc"], cur["fv"], np.asarray(has1, bool), s1, nb["kps"], nb["desc"], nb["fv"],
                                           nb["has"], s2, nb["F12"], nb["ex"], nb["ey"], scene["sf"], scene["sg"], False, False)[0]


def create_new_map_points(scene, masks=None):
    """The loop of LocalMapping.cc:281-517.  masks[k] (optional): the "owns a point" mask of the current keyframe to use in front
    of neighbour k instead of this loop's own (a test that follows another implementation's creations row by row).
    Returns dict(match12, status, x3d [K, n1(, 3)], gap [K, n1] (1 where no pair), A [K, n1, 16], from_svd, counts [K, NSTATUS], nnew)."""
    cur = scene["cur"]; K = len(scene["neigh"]); n1 = cur["n"]
    m12 = np.full((K, n1), -1, np.int32); st = np.full((K, n1), -1, np.int8); x3d = np.full((K, n1, 3), np.nan, np.float32)
    gap = np.ones((K, n1)); A = np.zeros((K, n1, 16), np.float32); from_svd = np.zeros((K, n1), bool)
    has1 = cur["has"].copy()
    for k in range(K):
        if masks is not None:
            has1 = np.asarray(masks[k], bool)
        st[k, has1] = STATUS["SKIPPED"]
        m = search(scene, k, has1)
        i1 = np.nonzero(m >= 0)[0]
        r = triangulate_pairs(scene, k, i1, m[i1])
        m12[k] = m
        st[k, i1] = r["status"]; gap[k, i1] = r["gap"]; A[k, i1] = r["A"]; from_svd[k, i1] = r["from_svd"] != 0
        made = r["status"] == STATUS["CREATED"]
        x3d[k, i1[made]] = r["x3d"][made]
        has1 = has1.copy(); has1[i1[made]] = True
    counts = np.stack([np.bincount(st[k][st[k] >= 0], minlength=NSTATUS) for k in range(K)]).astype(np.int32) if K else np.zeros((0, NSTATUS), np.int32)
    return dict(match12=m12, status=st, x3d=x3d, gap=gap, A=A, from_svd=from_svd, counts=counts, nnew=int((st == 0).sum()))


def null_vector_f64(A):
    """The float64 null vector (right singular vector of least singular value) of the float matrix A, dehomogenised"""
    v = np.linalg.svd(np.asarray(A, np.float64).reshape(4, 4))[2][3]
    return v[:3] / v[3]
