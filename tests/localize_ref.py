"""hostmath_localize (sift_amd/csrc/localize_math.h in a plain loop) and a Python float64 restatement of that header."""
import ctypes as C
import math

import numpy as np

import fund_ref as FR
from sift_amd import _lib
from sift_amd.synthetic import quadratic_stack   # noqa: F401 (the tests' exact stacks)

DTYPE = _lib.LOCALIZED_DTYPE
OK, SINGULAR, NOT_FINITE, LEFT_RANGE, NOT_CONVERGED = 0, 1, 2, 3, 4


def host(dogs, xs, ys, idx, max_moves=5, octave=0, coord_scale=1.0):
    """Records of hostmath_localize over one stack `dogs` [L, h, w]."""
    fn = FR.hostmath().hostmath_localize
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_void_p], None
    dogs = np.ascontiguousarray(dogs, np.float32)
    xs, ys, idx = (np.ascontiguousarray(a, np.uint16).reshape(-1) for a in (xs, ys, idx))
    out = np.zeros(xs.size, DTYPE)
    fn(dogs.ctypes.data, dogs.shape[0], dogs.shape[2], dogs.shape[1], xs.ctypes.data, ys.ctypes.data, idx.ctypes.data, xs.size, max_moves, octave,
       coord_scale, out.ctypes.data)
    return out


def batch_host(ctx, dogs, subpixel, images=None):
    """The host loop over the DoG levels read back from the context's last batch, image by image and octave by octave (max_moves 5)."""
    kp, _ = ctx.results()
    base = np.concatenate([[0], np.cumsum(ctx.counts())])
    want = np.zeros(kp.size, DTYPE)
    for img in range(base.size - 1) if images is None else images:
        k = kp[base[img]:base[img + 1]]
        for o in map(int, np.unique(k["octave"])):
            sel = np.flatnonzero(k["octave"] == o)
            want[base[img] + sel] = host(ctx.dog_stack(o, dogs, img), k["x"][sel], k["y"][sel], k["index"][sel], 5, o, 0.5 if subpixel else 1.0)
    return want


def _step(d):
    """One step on the 3 x 3 x 3 float64 block d[c, b, a] -> (status or None for a move, offset, gradient)."""
    if not np.isfinite(d).all():
        return NOT_FINITE, None, None
    p = d.tolist()   # Python floats: IEEE doubles, one rounding an operation
    d0 = p[1][1][1]
    gx, gy, gs = 0.5 * (p[1][1][2] - p[1][1][0]), 0.5 * (p[1][2][1] - p[1][0][1]), 0.5 * (p[2][1][1] - p[0][1][1])
    hxx, hyy, hss = (p[1][1][2] + p[1][1][0]) - (d0 + d0), (p[1][2][1] + p[1][0][1]) - (d0 + d0), (p[2][1][1] + p[0][1][1]) - (d0 + d0)
    hxy = 0.25 * ((p[1][2][2] - p[1][2][0]) - (p[1][0][2] - p[1][0][0]))
    hxs = 0.25 * ((p[2][1][2] - p[2][1][0]) - (p[0][1][2] - p[0][1][0]))
    hys = 0.25 * ((p[2][2][1] - p[2][0][1]) - (p[0][2][1] - p[0][0][1]))
    a00, a01, a02 = hyy * hss - hys * hys, hxs * hys - hxy * hss, hxy * hys - hxs * hyy
    a11, a12, a22 = hxx * hss - hxs * hxs, hxy * hxs - hxx * hys, hxx * hyy - hxy * hxy
    det = (hxx * a00 - hxy * (hxy * hss - hys * hxs)) + hxs * (hxy * hys - hyy * hxs)
    if det == 0.0 or not math.isfinite(det):
        return SINGULAR, None, None
    with np.errstate(all="ignore"):   # float64 scalars: an overflowing quotient is +-inf, as in C
        off = [float(-np.float64((r[0] * gx + r[1] * gy) + r[2] * gs) / np.float64(det)) for r in ((a00, a01, a02), (a01, a11, a12), (a02, a12, a22))]
    if not all(math.isfinite(o) for o in off):
        return NOT_FINITE, None, None
    return (OK if all(-0.5 <= o <= 0.5 for o in off) else None), off, (gx, gy, gs)


def restate(dogs, xs, ys, idx, max_moves=5, octave=0, coord_scale=1.0):
    """The same records from Python floats in the header's operation order."""
    dogs = np.ascontiguousarray(dogs, np.float32)
    out, f32, hi = np.zeros(len(xs), DTYPE), np.float32, (dogs.shape[2] - 2, dogs.shape[1] - 2, dogs.shape[0] - 2)
    for r, key in zip(out, zip(map(int, xs), map(int, ys), map(int, idx))):
        (x, y, i), moves = key, 0
        while True:
            d = dogs[i - 1:i + 2, y - 1:y + 2, x - 1:x + 2].astype(np.float64)
            status, off, g = _step(d)
            if status is None and moves >= max_moves:
                status = NOT_CONVERGED
            if status is None:
                new = tuple(p + (1 if o > 0.5 else -1 if o < -0.5 else 0) for p, o in zip((x, y, i), off))
                if all(1 <= p <= h for p, h in zip(new, hi)):
                    (x, y, i), moves = new, moves + 1
                    continue
                status = LEFT_RANGE
            break
        r["status"], r["moves"] = status, moves
        r["x"], r["y"], r["value"] = f32(key[0] << octave) * f32(coord_scale), f32(key[1] << octave) * f32(coord_scale), dogs[key[2], key[1], key[0]]
        if status == OK:
            scale = float(1 << octave) * float(coord_scale)
            with np.errstate(all="ignore"):
                r["x"], r["y"] = f32((float(x) + off[0]) * scale), f32((float(y) + off[1]) * scale)
                r["dx"], r["dy"], r["ds"] = (f32(o) for o in off)
                r["value"] = f32(float(d[1, 1, 1]) + 0.5 * ((g[0] * off[0] + g[1] * off[1]) + g[2] * off[2]))
            r["mx"], r["my"], r["mi"] = x - key[0], y - key[1], i - key[2]
    return out


def same(got, want):
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()
