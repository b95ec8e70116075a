"""hostmath_warp_homography (sift_amd/csrc/warp_math.h in a plain loop), a float64 numpy restatement of that header, and the
models the warp tests share.  A model maps an output (query-frame) point to a source point: (u, v, 1) ~ H (x, y, 1)."""
import ctypes as C
import math

import numpy as np

import fund_ref as FR
from sift_amd import _lib


def host(imgs, models, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp=1):
    """(out, mask) of the host loop; arguments as Context.warp_homography's, interp 0 / 1."""
    fn = FR.hostmath().hostmath_warp_homography
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(_lib.WarpParams), C.c_void_p, C.c_void_p], None
    imgs = np.ascontiguousarray(imgs, np.float32)
    models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
    src = None if src is None else np.ascontiguousarray(src, np.int32)
    oh, ow = imgs.shape[1:] if out_shape is None else out_shape
    out, mask = np.zeros((len(models), oh, ow), np.float32), np.zeros((len(models), oh, ow), np.uint8)
    prm = _lib.WarpParams(ow, oh, origin[0], origin[1], fill, interp, 0)
    fn(imgs.ctypes.data, imgs.shape[2], imgs.shape[1], len(models), None if src is None else src.ctypes.data, models.ctypes.data, C.byref(prm),
       out.ctypes.data, mask.ctypes.data)
    return out, mask


def restate(img, model, out_shape, origin=(0, 0)):
    """The definition in float64, bilinear: dict of u, v, W, the sums of magnitudes Sx, Sy, Sw, covered and value per output pixel."""
    img, (h, w) = np.asarray(img, np.float64), img.shape
    m = np.asarray(model, np.float32).astype(np.float64).reshape(9)
    qy, qx = np.mgrid[0:out_shape[0], 0:out_shape[1]].astype(np.float64)
    qx, qy = qx + origin[0], qy + origin[1]
    X, Y, W = (m[3 * r] * qx + m[3 * r + 1] * qy + m[3 * r + 2] for r in range(3))
    Sx, Sy, Sw = (abs(m[3 * r] * qx) + abs(m[3 * r + 1] * qy) + abs(m[3 * r + 2]) for r in range(3))
    with np.errstate(all="ignore"):
        u, v = X / W, Y / W
        covered = (W > 0) & np.isfinite(W) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    uc, vc = np.where(covered, u, 0.0), np.where(covered, v, 0.0)
    x0, y0 = np.floor(uc).astype(int), np.floor(vc).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = uc - x0, vc - y0
    top = img[y0, x0] + fx * (img[y0, x1] - img[y0, x0])
    bot = img[y1, x0] + fx * (img[y1, x1] - img[y1, x0])
    return dict(u=u, v=v, W=W, Sx=Sx, Sy=Sy, Sw=Sw, covered=covered, value=top + fy * (bot - top))


def translation(dx, dy):
    return [1, 0, dx, 0, 1, dy, 0, 0, 1]


def rot90(w):
    """np.rot90 of a w-wide image on an output of the transposed shape: (x, y) -> (w - 1 - y, x); integer entries, exact."""
    return [0, -1, w - 1, 1, 0, 0, 0, 0, 1]


def rotation(deg, scale, src_wh, out_wh):
    """Output centre -> source centre, then a rotation by `deg` and a scaling of the source step by `scale`."""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    (cx, cy), (ox, oy) = ((src_wh[0] - 1) / 2, (src_wh[1] - 1) / 2), ((out_wh[0] - 1) / 2, (out_wh[1] - 1) / 2)
    return [c, -s, cx - c * ox + s * oy, s, c, cy - s * ox - c * oy, 0, 0, 1]


def projective(base, a, b):
    """`base` with W = 1 + a x + b y."""
    return list(base[:6]) + [a, b, 1]


def job_models(w, h, ow, oh):
    """The GPU tests' job list: identity, half-pixel translation, 90 and 30 degree rotations, minification by 8, a projective model
    whose W changes sign inside the canvas, the null model and a NaN model."""
    rot30 = rotation(30.0, 0.75, (w, h), (ow, oh))
    return np.array([translation(0, 0), translation(0.5, 0.5), rot90(w), rot30, [8, 0, 0, 0, 8, 0, 0, 0, 1],
                     projective(rot30, -1.5 / max(ow, 2), -0.5 / max(oh, 2)), [0] * 9, [1, 0, 0, 0, float("nan"), 0, 0, 0, 1]], np.float32)
