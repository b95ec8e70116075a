"""hostmath_composite_homography (sift_amd/csrc/composite_math.h in a plain loop) and a float64 numpy blend over warp_ref.restate.
Jobs, models and images are warp_ref's; a canvas takes its jobs in order."""
import ctypes as C

import numpy as np

import fund_ref as FR
import warp_ref as WR
from sift_amd import _lib

BLENDS = ("first", "mean", "feather")


def host(imgs, models, offsets=None, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp=1, blend=2):
    """(out, count) of the host loop; arguments as Context.composite_homography's, interp 0 / 1, blend 0 / 1 / 2."""
    fn = FR.hostmath().hostmath_composite_homography
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.CompositeParams), C.c_void_p, C.c_void_p]
    fn.restype = None
    imgs = np.ascontiguousarray(imgs, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
    src = None if src is None else np.ascontiguousarray(src, np.int32)
    offsets = np.array([0, len(models)] if offsets is None else offsets, np.int64)
    oh, ow = imgs.shape[1:] if out_shape is None else out_shape
    out, count = np.zeros((len(offsets) - 1, oh, ow), np.float32), np.zeros((len(offsets) - 1, oh, ow), np.uint16)
    prm = _lib.CompositeParams(ow, oh, origin[0], origin[1], fill, interp, blend, 0)
    fn(imgs.ctypes.data, imgs.shape[2], imgs.shape[1], len(offsets) - 1, offsets.ctypes.data, None if src is None else src.ctypes.data, models.ctypes.data,
       C.byref(prm), out.ctypes.data, count.ctypes.data)
    return out, count


def blend64(imgs, models, out_shape, blend, origin=(0, 0)):
    """One canvas of job j = image j under models[j], bilinear, in float64 -> (value, cnt, wsum, jobs): jobs[j] is
    warp_ref.restate's dict with `wgt` added (the feather weight, 0 where not covered); value is NaN where cnt == 0."""
    h, w = imgs.shape[1:]
    jobs = [WR.restate(img, m, out_shape, origin) for img, m in zip(imgs, models)]
    for r in jobs:
        with np.errstate(all="ignore"):
            r["wgt"] = np.where(r["covered"], np.minimum(np.minimum(r["u"], w - 1 - r["u"]), np.minimum(r["v"], h - 1 - r["v"])) + 1.0, 0.0)
    cnt = sum(r["covered"].astype(int) for r in jobs)
    wsum = sum(r["wgt"] for r in jobs)
    first = np.full(out_shape, np.nan)
    for r in reversed(jobs):
        first = np.where(r["covered"], r["value"], first)
    with np.errstate(all="ignore"):
        mean = sum(np.where(r["covered"], r["value"], 0.0) for r in jobs) / cnt
        feather = sum(r["wgt"] * np.where(r["covered"], r["value"], 0.0) for r in jobs) / wsum
    return (first, mean, feather)[blend], cnt, wsum, jobs
