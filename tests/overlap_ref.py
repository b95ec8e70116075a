"""hostmath_overlap_stats and hostmath_composite_homography_gains (sift_amd/csrc/overlap_math.h, composite_math.h in plain loops)
and a numpy reference of the statistics and gains over the host warp loop (warp_ref.host).  Jobs and models are warp_ref's."""
import ctypes as C
import functools

import numpy as np

import fund_ref as FR
import warp_ref as WR
from sift_amd import _lib
from sift_amd.synthetic import synth_frame

ORIGIN, OFFSETS = (-2, 1), [0, 5, 5, 8]
SHAPES = [(1, 1, 1, 1), (5, 3, 7, 2), (65, 17, 63, 33)]


def _args(imgs, models, offsets, src):
    imgs = np.ascontiguousarray(imgs, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
    src = None if src is None else np.ascontiguousarray(src, np.int32)
    offsets = np.array([0, len(models)] if offsets is None else offsets, np.int64)
    return imgs, models, offsets, src, (imgs.ctypes.data, imgs.shape[2], imgs.shape[1], len(offsets) - 1, offsets.ctypes.data,
                                        None if src is None else src.ctypes.data, models.ctypes.data)


def host(imgs, models, offsets=None, src=None, out_shape=None, origin=(0, 0), scale=1.0, interp=1, sigma_n=10.0, sigma_g=0.1):
    """(stats, gains, status) of the host loop; arguments as Context.overlap_stats's, interp 0 / 1."""
    fn = FR.hostmath().hostmath_overlap_stats
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.POINTER(_lib.OverlapParams)] + [C.c_void_p] * 3, None
    imgs, models, offsets, src, head = _args(imgs, models, offsets, src)
    oh, ow = imgs.shape[1:] if out_shape is None else out_shape
    stats, gains = np.zeros((len(offsets) - 1, 4, 32, 32), np.int64), np.ones(len(models), np.float32)
    status = np.zeros(len(offsets) - 1, np.uint8)
    prm = _lib.OverlapParams(ow, oh, origin[0], origin[1], scale, sigma_n, sigma_g, interp, 0)
    fn(*head, C.byref(prm), stats.ctypes.data, gains.ctypes.data, status.ctypes.data)
    return stats, gains, status


def host_composite(imgs, models, gains, offsets=None, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp=1, blend=2):
    """(out, count) of the host loop with gains; arguments as composite_ref.host's."""
    fn = FR.hostmath().hostmath_composite_homography_gains
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.POINTER(_lib.CompositeParams)] + [C.c_void_p] * 3, None
    imgs, models, offsets, src, head = _args(imgs, models, offsets, src)
    gains = np.ascontiguousarray(gains, np.float32)
    oh, ow = imgs.shape[1:] if out_shape is None else out_shape
    out, count = np.zeros((len(offsets) - 1, oh, ow), np.float32), np.zeros((len(offsets) - 1, oh, ow), np.uint16)
    prm = _lib.CompositeParams(ow, oh, origin[0], origin[1], fill, interp, blend, 0)
    fn(*head, C.byref(prm), gains.ctypes.data, out.ctypes.data, count.ctypes.data)
    return out, count


def numpy_stats(imgs, models, src=None, out_shape=None, origin=(0, 0), scale=1.0, interp=1):
    """One canvas of all jobs -> [4, 32, 32] int64 from the host warp's values and masks."""
    val, mask = WR.host(imgs, models, src, out_shape, origin, 0.0, interp)
    n = len(val)
    t = (val.reshape(n, -1).astype(np.float64) * scale + 0.5).astype(np.float32)
    c = mask.reshape(n, -1).astype(np.int64)
    q = c * np.where(t >= 0, np.minimum(np.floor(t), 255), 0).astype(np.int64)
    stats = np.zeros((4, 32, 32), np.int64)
    for k, (a, b) in enumerate([(c, c), (q, c), (q * q, c), (q, q)]):
        stats[k, :n, :n] = np.einsum("ip,jp->ij", a, b)
    return stats


def numpy_gains(stats, n, sigma_n=10.0, sigma_g=0.1):
    """numpy.linalg.solve in float64 on the normal equations of overlap_math.h."""
    N, S = stats[0, :n, :n].astype(np.float64), stats[1, :n, :n].astype(np.float64)
    alpha, beta = 1.0 / sigma_n ** 2, 1.0 / sigma_g ** 2
    with np.errstate(all="ignore"):
        I = np.where(N > 0, S / N, 0.0)
    off = 1.0 - np.eye(n)
    A = -2 * alpha * I * I.T * N * off + np.diag((beta * N + 2 * alpha * I * I * N * off).sum(axis=1))
    b = beta * N.sum(axis=1)
    for i in np.flatnonzero(np.diag(N) == 0):
        A[i], b[i] = np.eye(n)[i], 1.0
    return np.linalg.solve(A, b) if n else np.zeros(0)


@functools.lru_cache(maxsize=None)
def case(w, h, ow, oh, interp):
    """composite_ref's jobs: two images, WR.job_models' eight models in three groups, the middle one empty, and the host loop's result."""
    imgs = (np.random.default_rng(w + 31 * h).random((2, h, w)) * 255).astype(np.float32)
    models, src = WR.job_models(w, h, ow, oh), np.arange(8, dtype=np.int32) % 2
    return imgs, models, src, host(imgs, models, OFFSETS, src, (oh, ow), ORIGIN, 1.0, interp)


@functools.lru_cache(maxsize=None)
def exposure_fixture():
    """Three 96 x 64 cuts of one synthetic frame at x-steps of 24, exposed by 0.8, 1.0 and 1.25, under their exact translations,
    on the canvas that holds them all -> (imgs, models, (out_h, out_w))."""
    big = synth_frame(160, 64, 1).astype(np.float32)
    imgs = np.stack([np.ascontiguousarray(big[:, 24 * k:24 * k + 96]) * np.float32(g) for k, g in enumerate((0.8, 1.0, 1.25))])
    return imgs, np.array([WR.translation(-24 * k, 0) for k in range(3)], np.float32), (64, 144)


def exposure_residual(stats, gains, n=3):
    """max over overlapping pairs of |g_i I_ij - g_j I_ji|"""
    N, S = stats[0, :n, :n].astype(np.float64), stats[1, :n, :n].astype(np.float64)
    return max(abs(gains[i] * S[i, j] / N[i, j] - gains[j] * S[j, i] / N[j, i]) for i in range(n) for j in range(n) if i != j and N[i, j] > 0)
