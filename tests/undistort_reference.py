"""Frame::UndistortKeyPoints / ComputeImageBounds restated in numpy float64, for the undistortion tests: what
cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) of OpenCV 3.4 computes for CV_32FC2 points (orb_slam2_e_amd/csrc/
orbm_undistort.h states the same sequence for the host and the device).  Element-wise operations only, in the written order, so
every operation rounds once, as the IEEE double + - * / of the C code do.  Also the forward distortion model (the first-principles
check of the inverse) and the cameras of the tests, typed in as data."""
import numpy as np

# name -> ((fx, fy, cx, cy, k1, k2, p1, p2, k3), (width, height)).  The first two are launch files of the reference (Camera.* as
# written there, four coefficients: k3 = 0); the size of the sHamlyn04 image is the tests' choice (the launch file gives none).
CAMERAS = {
    "sHamlyn04": ((752.737796, 765.331797, 263.657845, 245.883296, -0.332222, 0.708196, 0.003904, 0.008043, 0.0), (640, 480)),
    "sHCULB_00053": ((364.6158, 365.0793, 368.1022, 271.2141, -0.1264694, -0.006895169, 0.001731781, -0.00007914314, 0.0), (720, 540)),
    "synthetic_k3": ((520.5, 517.25, 318.75, 243.5, -0.2815, 0.0931, 0.00071, -0.00034, -0.0127), (640, 480)),
}


def widen(cam):
    """the nine camera numbers as the library holds them (floats), widened to double"""
    return [np.float64(np.float32(v)) for v in cam]


def normalised(cam, xy):
    """the five iterations: (x, y) in normalised coordinates, float64, of float32 pixels xy[n][2]"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = widen(cam)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    px, py = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        ifx = 1.0 / fx; ify = 1.0 / fy
        x0 = (px - cx) * ifx; y0 = (py - cy) * ify
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dX) * icdist; y = (y0 - dY) * icdist
    return x, y


def undistort(cam, xy):
    """mvKeysUn coordinates, float32 [n][2].  k1 == 0: the input (src/Frame.cc:421-425 tests k1 only)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    if np.float32(cam[4]) == 0:
        return xy.copy()
    fx, fy, cx, cy = widen(cam)[:4]
    x, y = normalised(cam, xy)
    with np.errstate(all="ignore"):
        return np.stack([(fx * x + cx).astype(np.float32), (fy * y + cy).astype(np.float32)], 1)


def image_bounds(cam, width, height):
    """(mnMinX, mnMinY, mnMaxX, mnMaxY), float32: the four corners with min / max as src/Frame.cc:466-469 take them"""
    if np.float32(cam[4]) == 0:
        return np.array([0, 0, width, height], np.float32)
    c = undistort(cam, np.array([[0, 0], [width, 0], [0, height], [width, height]], np.float32))
    return np.array([min(c[0, 0], c[2, 0]), min(c[0, 1], c[1, 1]), max(c[1, 0], c[3, 0]), max(c[2, 1], c[3, 1])], np.float32)


def distort(cam, x, y):
    """The forward model: normalised undistorted (x, y) -> distorted pixel (float64)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = widen(cam)
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def sample_points(cam, size, n, seed=0):
    """n float32 points of a width x height image: the principal point, the four corners, integer and .5 coordinates, then
    uniform ones (the first n of that list)."""
    w, h = size
    rng = np.random.default_rng(seed)
    fixed = [[np.float32(cam[2]), np.float32(cam[3])], [0, 0], [w, 0], [0, h], [w, h], [17, 230], [400, 3], [100.5, 200.5], [0.5, h - 0.5]]
    pts = np.concatenate([np.array(fixed, np.float32), (rng.random((max(n, 1), 2)) * [w, h]).astype(np.float32)])
    return np.ascontiguousarray(pts[:n])



def same_bits_or_both_not_finite(a, b):
    """float32 arrays: equal bits where both are finite, and not finite in the same places"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    fa, fb = np.isfinite(a), np.isfinite(b)
    return a.shape == b.shape and np.array_equal(fa, fb) and np.array_equal(a[fa].view(np.uint32), b[fb].view(np.uint32))
