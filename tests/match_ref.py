"""Shared by tests/test_match_host.py and tests/test_match_gpu.py: the host checker of descriptor matching
(hostmath_match_knn2 in libsift_hostmath.so: the definition of include/sift_hip.h as plain fmaf loops), the numpy filter
over its top-2, and the row generators."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = None


def hostmath():
    global _H
    if _H is None:
        path = os.path.join(ROOT, "sift_amd", "lib", "libsift_hostmath.so")
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sift_amd", "csrc"), "../lib/libsift_hostmath.so"])
        _H = C.CDLL(path)
        vp = C.c_void_p
        _H.hostmath_match_knn2.argtypes = [vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp]
        _H.hostmath_match_knn2.restype = None
    return _H


def knn2(q, t, q_valid=None, t_valid=None):
    """(idx [nq, 2] int32, dist2 [nq, 2] float32) by the checker."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
    qv = None if q_valid is None else np.ascontiguousarray(q_valid, np.uint8)
    tv = None if t_valid is None else np.ascontiguousarray(t_valid, np.uint8)
    idx = np.zeros((q.shape[0], 2), np.int32)
    dist = np.zeros((q.shape[0], 2), np.float32)
    hostmath().hostmath_match_knn2(q.ctypes.data, None if qv is None else qv.ctypes.data, q.shape[0], t.ctypes.data,
                                   None if tv is None else tv.ctypes.data, t.shape[0], idx.ctypes.data, dist.ctypes.data)
    return idx, dist


def filter_matches(idx, dist, ratio, cross_check, rev_idx=None):
    """The records sift_hip_match must deliver for one pair, from the checker's top-2 (rev_idx: the top-2 with the roles
    swapped).  All arithmetic in float32: (ratio * ratio) and its product with the second distance are single multiplies."""
    n = idx.shape[0]
    keep = idx[:, 0] >= 0
    if ratio != 0:
        r2 = np.float32(ratio) * np.float32(ratio)
        with np.errstate(invalid="ignore"):
            keep &= dist[:, 0] < (r2 * dist[:, 1]).astype(np.float32)
    if cross_check:
        best = np.where(idx[:, 0] >= 0, idx[:, 0], 0)
        back = rev_idx[best, 0] if rev_idx.shape[0] else np.full(n, -2)
        keep &= back == np.arange(n)
    rec = np.zeros(int(keep.sum()), [("query", "<i4"), ("train", "<i4"), ("dist2", "<f4"), ("second2", "<f4")])
    rec["query"] = np.nonzero(keep)[0]
    rec["train"] = idx[keep, 0]
    rec["dist2"] = dist[keep, 0]
    rec["second2"] = dist[keep, 1]
    return rec


def desc_rows(rng, n):
    """Descriptor-shaped rows: non-negative, 16 cells of 8 bins each summing to 1, bin 7 zero, about two thirds zeros."""
    v = rng.random((n, 16, 8)).astype(np.float32)
    v *= rng.random((n, 16, 8)) < 0.38
    v[:, :, 7] = 0
    empty = v.sum(axis=2) == 0
    v[:, :, 0] += empty            # a cell with nothing in it gets its first bin
    v /= v.sum(axis=2, keepdims=True, dtype=np.float32)
    return np.ascontiguousarray(v.reshape(n, 128), np.float32)


def uniform_rows(rng, n):
    return np.ascontiguousarray(rng.random((n, 128), np.float32) * np.float32(2) - np.float32(1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
