"""Shared by tests/test_match_u8_host.py and tests/test_match_u8_gpu.py: the host checker of 8-bit descriptor matching
(hostmath_quantize and hostmath_match_knn2_u8 in libsift_hostmath.so: the definition of include/sift_hip.h, "8-bit descriptors and
integer matching", as plain loops), numpy restatements of both that share no code with them, and the row generators."""
import ctypes as C

import numpy as np

import match_ref as M

_DECLARED = False

# not-a-number, the infinities, signed zero, a tiny negative, subnormals, 0, 1, 1 + ulp, 2, 1e30 - and what the quantiser makes of them
KAT_IN = np.array([np.nan, np.inf, -np.inf, -0.0, -1e-30, 1e-45, -1e-45, 1e-39, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, 1e30],
                  np.float32)
KAT_OUT = np.array([0, 255, 0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255], np.uint8)


def hostmath():
    global _DECLARED
    H = M.hostmath()
    if not _DECLARED:
        vp = C.c_void_p
        H.hostmath_quantize.argtypes = [vp, C.c_longlong, vp]
        H.hostmath_quantize.restype = None
        H.hostmath_match_knn2_u8.argtypes = [vp, vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp]
        H.hostmath_match_knn2_u8.restype = None
        _DECLARED = True
    return H


def quantize(desc):
    """[n, 128] uint8 by the checker (any float32 array whose size is a multiple of 128)."""
    d = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
    out = np.zeros(d.shape, np.uint8)
    hostmath().hostmath_quantize(d.ctypes.data, d.shape[0], out.ctypes.data)
    return out


def quantize_flat(v):
    """The checker over any number of floats (padded to whole rows)."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    pad = (-v.size) % 128
    return quantize(np.concatenate([v, np.zeros(pad, np.float32)])).reshape(-1)[:v.size]


def quantize_np(v):
    """The quantiser restated in numpy: t = fmaf(v, 255, 0.5) is the float64 value rounded ONCE to float32 - v * 255 is exact
    in float64 (24 + 8 bits), and adding 0.5 is exact there unless the product is below 2^-22; then t lies within 2^-21 of 0.5
    under either rounding and q is 0."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v.astype(np.float64) * 255.0 + 0.5).astype(np.float32)
        q = np.where(t >= np.float32(255), 255, np.where(t >= np.float32(0), np.trunc(np.where(np.isfinite(t), t, 0)), 0))
    return q.astype(np.uint8)


def knn2(q, t, q_valid=None, t_valid=None):
    """(idx [nq, 2] int32, dist2 [nq, 2] float32) by the checker, over uint8 rows."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 128)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 128)
    qv = None if q_valid is None else np.ascontiguousarray(q_valid, np.uint8)
    tv = None if t_valid is None else np.ascontiguousarray(t_valid, np.uint8)
    idx = np.zeros((q.shape[0], 2), np.int32)
    dist = np.zeros((q.shape[0], 2), np.float32)
    hostmath().hostmath_match_knn2_u8(q.ctypes.data, None if qv is None else qv.ctypes.data, q.shape[0], t.ctypes.data,
                                      None if tv is None else tv.ctypes.data, t.shape[0], idx.ctypes.data, dist.ctypes.data)
    return idx, dist


def dist_matrix(q, t):
    """sum (a - b)^2 of every (query row, train row) in int64."""
    qi = np.asarray(q).reshape(-1, 128).astype(np.int64)
    ti = np.asarray(t).reshape(-1, 128).astype(np.int64)
    return (qi * qi).sum(axis=1)[:, None] + (ti * ti).sum(axis=1)[None, :] - 2 * qi @ ti.T


def knn2_np(q, t, q_valid=None, t_valid=None):
    """The same by an int64 numpy brute force: a stable sort of the distance matrix is the order (d2, index)."""
    d = dist_matrix(q, t)
    nq, nt = d.shape
    big = np.int64(1) << 40
    if t_valid is not None:
        d = np.where(np.asarray(t_valid)[None, :] != 0, d, big)
    if q_valid is not None:
        d = np.where(np.asarray(q_valid)[:, None] != 0, d, big)
    d = np.concatenate([d, np.full((nq, 2), big)], axis=1)            # two missing entries behind every row
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    dd = np.take_along_axis(d, order, axis=1)
    idx = np.where(dd < big, order, -1).astype(np.int32)
    with np.errstate(over="ignore"):
        dist = np.where(dd < big, dd.astype(np.float32), np.float32(np.inf)).astype(np.float32)
    return idx, dist


def desc_rows_u8(rng, n):
    return quantize(M.desc_rows(rng, n))


def uniform_rows_u8(rng, n):
    return rng.integers(0, 256, (n, 128), dtype=np.uint8)


EXTREMES = np.stack([np.zeros(128, np.uint8), np.full(128, 255, np.uint8), np.full(128, 127, np.uint8), np.full(128, 128, np.uint8),
                     np.tile(np.array([0, 255], np.uint8), 64)])
