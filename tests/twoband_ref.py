"""hostmath_composite_twoband (sift_amd/csrc/twoband_math.h in a plain loop) and a float64 numpy restatement of that header:
composite_ref.blend64's jobs on the canvas widened by the radius, two passes of shifted sums, bands and blend."""
import ctypes as C

import numpy as np

import composite_ref as CR
import fund_ref as FR
from sift_amd import _lib


def host(imgs, models, taps, offsets=None, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp=1, gains=None):
    """(out, count) of the host loop; arguments as Context.composite_twoband's, interp 0 / 1."""
    fn = FR.hostmath().hostmath_composite_twoband
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.TwobandParams), C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p]
    fn.restype = None
    imgs = np.ascontiguousarray(imgs, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
    taps = np.ascontiguousarray(taps, np.float32)
    src = None if src is None else np.ascontiguousarray(src, np.int32)
    gains = None if gains is None else np.ascontiguousarray(gains, np.float32)
    offsets = np.array([0, len(models)] if offsets is None else offsets, np.int64)
    oh, ow = imgs.shape[1:] if out_shape is None else out_shape
    out, count = np.zeros((len(offsets) - 1, oh, ow), np.float32), np.zeros((len(offsets) - 1, oh, ow), np.uint16)
    prm = _lib.TwobandParams(ow, oh, origin[0], origin[1], fill, interp, 0, len(taps) - 1)
    fn(imgs.ctypes.data, imgs.shape[2], imgs.shape[1], len(offsets) - 1, offsets.ctypes.data, None if src is None else src.ctypes.data, models.ctypes.data,
       C.byref(prm), taps.ctypes.data, None if gains is None else gains.ctypes.data, out.ctypes.data, count.ctypes.data)
    return out, count


def chain(a, taps, axis, rnd):
    """One pass: the sums over d = -R .. R ascending of taps[|d|] * a shifted by d along `axis`, which loses R at either end."""
    R, n = len(taps) - 1, a.shape[axis] - 2 * (len(taps) - 1)
    acc = np.zeros(np.take(a, range(n), axis).shape)
    for d in range(-R, R + 1):
        acc = rnd(float(taps[abs(d)]) * np.take(a, range(R + d, R + d + n), axis) + acc)
    return acc


def twoband64(imgs, models, taps, out_shape, origin=(0, 0), gains=None, rnd=lambda a: a):
    """One canvas of job j = image j under models[j], bilinear, in float64 -> (value, cnt, jobs): jobs[j] holds composite_ref.blend64's
    fields on the canvas widened by R (`wide`) and covered, wgt, t, L, H on the canvas; value is NaN where cnt == 0.  `rnd` is applied
    after every operation the header defines: the identity, or a rounding to float32 where every operation is exact in float64 before it."""
    R, (oh, ow) = len(taps) - 1, out_shape
    wide = CR.blend64(imgs, models, (oh + 2 * R, ow + 2 * R), 2, (origin[0] - R, origin[1] - R))[3]
    crop = lambda a: a[R:R + oh, R:R + ow]
    lacc, wsum, best, high = (np.zeros(out_shape) for _ in range(4))
    cnt, jobs = np.zeros(out_shape, int), []
    for j, r in enumerate(wide):
        t = np.where(r["covered"], r["value"], 0.0)
        t = t if gains is None else rnd(float(np.float32(gains[j])) * t)
        ls = chain(chain(t, taps, 1, rnd), taps, 0, rnd)
        ln = chain(chain(r["covered"].astype(np.float64), taps, 1, rnd), taps, 0, rnd)
        c, wgt = crop(r["covered"]), crop(r["wgt"])
        with np.errstate(all="ignore"):
            L = rnd(ls / ln)
        H = rnd(crop(t) - L)
        lacc, wsum = np.where(c, rnd(wgt * np.where(c, L, 0.0) + lacc), lacc), np.where(c, rnd(wsum + wgt), wsum)
        take = c & ((cnt == 0) | (wgt > best))
        best, high, cnt = np.where(take, wgt, best), np.where(take, H, high), cnt + c
        jobs.append(dict(wide=r, covered=c, wgt=wgt, t=crop(t), L=L, H=H))
    with np.errstate(all="ignore"):
        value = np.where(cnt > 0, rnd(rnd(lacc / wsum) + high), np.nan)
    return value, cnt, jobs
