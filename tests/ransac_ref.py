"""Shared by tests/test_ransac_host.py and tests/test_ransac_gpu.py: the host checker of the geometric verification
(hostmath_ransac_homography and its pieces in libsift_hostmath.so: sift_amd/csrc/ransac_math.h in plain loops) and the
generators of correspondences."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_DTYPE = np.dtype([("h", "<f4", (9,)), ("inliers", "<i4"), ("iteration", "<i4"), ("reserved", "<i4")])
assert MODEL_DTYPE.itemsize == 48
_H = None


def hostmath():
    global _H
    if _H is None:
        path = os.path.join(ROOT, "sift_amd", "lib", "libsift_hostmath.so")
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sift_amd", "csrc"), "../lib/libsift_hostmath.so"])
        _H = C.CDLL(path)
        vp, u32 = C.c_void_p, C.c_uint32
        _H.hostmath_ransac_draw.argtypes = [u32, u32, u32, u32, vp]
        _H.hostmath_ransac_draw.restype = None
        _H.hostmath_homography4.argtypes = [vp, vp]
        _H.hostmath_ransac_inlier.argtypes = [vp, vp, C.c_float]
        _H.hostmath_ransac_homography.argtypes = [vp, C.c_int, vp, u32, u32, C.c_float, vp, vp, vp]
        _H.hostmath_ransac_homography.restype = None
    return _H


def draw(seed, set_, iteration, m):
    idx = np.zeros(4, np.uint32)
    hostmath().hostmath_ransac_draw(seed, set_, iteration, m, idx.ctypes.data)
    return idx


def draws(seed, set_, iterations, m):
    return np.stack([draw(seed, set_, i, m) for i in range(iterations)])


def homography4(rows):
    """(valid, h [9] float32) of four correspondences (qx, qy, tx, ty)."""
    c = np.ascontiguousarray(rows, np.float32).reshape(4, 4)
    h = np.full(9, 7, np.float32)
    ok = hostmath().hostmath_homography4(c.ctypes.data, h.ctypes.data)
    return bool(ok), h


def inlier(h, row, thr):
    h = np.ascontiguousarray(h, np.float32)
    row = np.ascontiguousarray(row, np.float32)
    return bool(hostmath().hostmath_ransac_inlier(h.ctypes.data, row.ctypes.data, thr))


def ransac(pts, offsets=None, iterations=2048, threshold=3.0, seed=0):
    """(models [n_sets] MODEL_DTYPE, inlier [rows] uint8, scores [n_sets, iterations] int32) by the checker."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    offsets = np.array([0, pts.shape[0]], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
    n = offsets.size - 1
    models = np.zeros(n, MODEL_DTYPE)
    flags = np.zeros(pts.shape[0], np.uint8)
    scores = np.zeros((n, iterations), np.int32)
    hostmath().hostmath_ransac_homography(pts.ctypes.data, n, offsets.ctypes.data, iterations, seed, threshold, models.ctypes.data,
                                          flags.ctypes.data, scores.ctypes.data)
    return models, flags, scores


def apply_h(H, xy):
    """float64 projection of points [n, 2] by a 3 x 3 matrix."""
    p = np.concatenate([np.asarray(xy, np.float64), np.ones((len(xy), 1))], axis=1) @ np.asarray(H, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:3]


H_PROJ = np.array([[0.9, 0.08, 30.0], [-0.05, 1.1, -12.0], [4e-5, -3e-5, 1.0]])


def projective_rows(rng, m, outliers=0.6, H=H_PROJ, size=1000.0, noise=0.0):
    """m correspondences under H, a share of them with uniform random targets -> (rows float32, true error in pixels float64).
    The query points are integers, like keypoint coordinates."""
    q = np.floor(rng.random((m, 2)) * size)
    t = apply_h(H, q) + noise * rng.standard_normal((m, 2))
    bad = rng.random(m) < outliers
    t[bad] = rng.random((int(bad.sum()), 2)) * size
    rows = np.ascontiguousarray(np.concatenate([q, t], axis=1), np.float32)
    err = np.sqrt(((apply_h(H, rows[:, :2]) - rows[:, 2:].astype(np.float64)) ** 2).sum(axis=1))
    return rows, err


def random_rows(rng, m, size=1000.0):
    return np.ascontiguousarray(rng.random((m, 4)) * size, np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
