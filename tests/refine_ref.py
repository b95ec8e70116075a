"""Shared by tests/test_refine_host.py and tests/test_refine_gpu.py: the host checker of the RANSAC refinement
(hostmath_refine_homography and its pieces in libsift_hostmath.so: sift_amd/csrc/ransac_refine_math.h in plain loops), a numpy
restatement of its fixed-order sums, and helpers.  The generators and the unrefined checker are tests/ransac_ref.py's."""
import ctypes as C

import numpy as np

import ransac_ref as R

MODEL_DTYPE = np.dtype([("h", "<f4", (9,)), ("inliers", "<i4"), ("iteration", "<i4"), ("refined", "<i4")])
assert MODEL_DTYPE.itemsize == 48
CORNERS = np.array([[0, 0], [1000, 0], [1000, 1000], [0, 1000]], np.float64)   # the 1000 px square of the generators
_BOUND = False


def hostmath():
    global _BOUND
    H = R.hostmath()
    if not _BOUND:
        vp, u32 = C.c_void_p, C.c_uint32
        H.hostmath_refine_homography.argtypes = [vp, C.c_int, vp, C.c_float, C.c_int, vp, vp]
        H.hostmath_refine_homography.restype = None
        H.hostmath_ransac_homography_refined.argtypes = [vp, C.c_int, vp, u32, u32, C.c_float, vp, vp, vp, C.c_int]
        H.hostmath_ransac_homography_refined.restype = None
        H.hostmath_refine_sums.argtypes = [vp, C.c_longlong, vp, C.c_float, vp]
        H.hostmath_refine_normalisation.argtypes = [vp, C.c_int, vp]
        H.hostmath_solve8.argtypes = [vp, vp, vp]
        _BOUND = True
    return H


def _sets(pts, offsets):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    offsets = np.array([0, pts.shape[0]], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
    return pts, offsets


def ransac(pts, offsets=None, iterations=2048, threshold=3.0, seed=0, refine=0):
    """(models [n_sets] MODEL_DTYPE, inlier [rows] uint8, scores [n_sets, iterations] int32) by the checker, refined."""
    pts, offsets = _sets(pts, offsets)
    n = offsets.size - 1
    models = np.zeros(n, MODEL_DTYPE)
    flags = np.zeros(pts.shape[0], np.uint8)
    scores = np.zeros((n, iterations), np.int32)
    hostmath().hostmath_ransac_homography_refined(pts.ctypes.data, n, offsets.ctypes.data, iterations, seed, threshold, models.ctypes.data,
                                                  flags.ctypes.data, scores.ctypes.data, refine)
    return models, flags, scores


def refine(pts, models, offsets=None, threshold=3.0, rounds=2):
    """(models, inlier) of hostmath_refine_homography from the given models (copied)."""
    pts, offsets = _sets(pts, offsets)
    models = np.array(models, MODEL_DTYPE).reshape(-1)
    assert models.size == offsets.size - 1
    flags = np.full(pts.shape[0], 7, np.uint8)
    hostmath().hostmath_refine_homography(pts.ctypes.data, models.size, offsets.ctypes.data, threshold, rounds, models.ctypes.data, flags.ctypes.data)
    return models, flags


def model_of(H, iteration=0):
    """One MODEL_DTYPE record holding the 3 x 3 matrix H (rounded to float) as a caller-supplied model."""
    m = np.zeros(1, MODEL_DTYPE)
    m["h"][0] = np.asarray(H, np.float64).ravel().astype(np.float32)
    m["iteration"] = iteration
    m["inliers"] = -5      # ignored and rewritten
    m["refined"] = 77      # likewise
    return m


def refine_sums(pts, h, threshold=3.0):
    """(n, sums [28] float64): n as hostmath_refine_sums returns it (-1 - n when the round fails before the normal sums)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    h = np.ascontiguousarray(h, np.float32)
    out = np.full(28, np.nan, np.float64)
    n = hostmath().hostmath_refine_sums(pts.ctypes.data, pts.shape[0], h.ctypes.data, threshold, out.ctypes.data)
    return n, out


def normalisation(mom, n):
    mom = np.ascontiguousarray(mom, np.float64)
    out = np.zeros(6, np.float64)
    ok = hostmath().hostmath_refine_normalisation(mom.ctypes.data, n, out.ctypes.data)
    return bool(ok), out


def solve8(a, b):
    a = np.ascontiguousarray(a, np.float64).reshape(8, 8)
    b = np.ascontiguousarray(b, np.float64).reshape(8)
    x = np.zeros(8, np.float64)
    ok = hostmath().hostmath_solve8(a.ctypes.data, b.ctypes.data, x.ctypes.data)
    return bool(ok), x


def fixed_order_sum(terms, rows):
    """The definition restated in numpy float64: `terms` [k, n_terms] of the inlier rows `rows` (ascending row numbers) ->
    256 partials, partial p the sequential sum from +0.0 of the rows i = p (mod 256), then the adjacent pairwise tree."""
    terms = np.asarray(terms, np.float64)
    s = np.zeros((256, terms.shape[1]), np.float64)
    for t, i in zip(terms, rows):
        s[i % 256] = s[i % 256] + t
    w = 1
    while w < 256:
        s[0::2 * w] = s[0::2 * w] + s[w::2 * w]
        w *= 2
    return s[0]


def corner_error(h, H=R.H_PROJ):
    """Largest distance in pixels between the images of the 1000 px square's corners under h and under H."""
    d = R.apply_h(np.asarray(h, np.float64), CORNERS) - R.apply_h(H, CORNERS)
    return float(np.sqrt((d ** 2).sum(axis=1)).max())
