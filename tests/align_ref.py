"""hostmath_align_homography / hostmath_align_sums (sift_amd/csrc/align_math.h in plain loops), a float64 numpy Gauss-Newton of the
same objective - the same contributing set, bilinear gradient, gauge and acceptance rule, no fixed order - and the analytic
fixture the alignment tests share."""
import ctypes as C
import functools
import math

import numpy as np

import fund_ref as FR
from sift_amd import _lib

I, J = np.triu_indices(12)   # entry e of the 78 sums is column I[e] times column J[e]


def _fn(name, argtypes):
    fn = getattr(FR.hostmath(), name)
    fn.argtypes, fn.restype = argtypes, None
    return fn


def records(models, iteration=0):
    rec = np.zeros(len(models), _lib.HOMOGRAPHY_DTYPE)
    rec["h"], rec["iteration"] = np.asarray(models, np.float32).reshape(-1, 9), iteration
    return rec


def host(imgs, pairs, models, rounds=4, border=2, min_pixels=256, damping=0.0):
    """(models, out, sums) of the host loop; `models`: HOMOGRAPHY_DTYPE records (copied)."""
    vp, ci = C.c_void_p, C.c_int
    fn = _fn("hostmath_align_homography", [vp, ci, ci, ci, vp, vp, C.POINTER(_lib.AlignParams), vp, vp, vp])
    imgs, models = np.ascontiguousarray(imgs, np.float32), np.array(models, _lib.HOMOGRAPHY_DTYPE).reshape(-1)
    pq, pt = (np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2)[:, k]) for k in (0, 1))
    out, sums = np.zeros(len(models), _lib.ALIGNMENT_DTYPE), np.zeros((len(models), _lib.ALIGN_SUMS))
    prm = _lib.AlignParams(rounds, border, min_pixels, damping, 0)
    fn(imgs.ctypes.data, imgs.shape[2], imgs.shape[1], len(models), pq.ctypes.data, pt.ctypes.data, C.byref(prm), models.ctypes.data, out.ctypes.data,
       sums.ctypes.data)
    return models, out, sums


def host_sums(imgs, model, gain=1.0, bias=0.0, border=2):
    """The 80 sums of the pair (0, 1) of `imgs` at (model, gain, bias) in the header's order."""
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    fn = _fn("hostmath_align_sums", [vp, ci, ci, ci, ci, vp, cf, cf, ci, vp])
    imgs, m, sums = np.ascontiguousarray(imgs, np.float32), np.ascontiguousarray(model, np.float32).reshape(9), np.zeros(_lib.ALIGN_SUMS)
    fn(imgs.ctypes.data, imgs.shape[2], imgs.shape[1], 0, 1, m.ctypes.data, gain, bias, border, sums.ctypes.data)
    return sums


def norm(w, h):
    """(cx, cy, s): the frame centre and the power-of-two scale of align_norm."""
    return (w - 1) / 2, (h - 1) / 2, 2.0 ** -(math.floor(math.log2((w * w + h * h) / 12)) // 2)


def gram64(Q, T, H, a=1.0, b=0.0, border=2):
    """(G [12, 12], n): the Gram matrix of the twelve columns over the contributing pixels, all in float64."""
    Q, T, (h, w) = np.asarray(Q, np.float64), np.asarray(T, np.float64), Q.shape
    m, (cx, cy, s) = np.asarray(H, np.float64).reshape(9), norm(w, h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    X, Y, W = (m[3 * r] * x + m[3 * r + 1] * y + m[3 * r + 2] for r in range(3))
    with np.errstate(all="ignore"):
        u, v = X / W, Y / W
        on = (W > 0) & np.isfinite(W) & (u >= 0) & (u < w - 1) & (v >= 0) & (v < h - 1)
    on &= (x >= border) & (x <= w - 1 - border) & (y >= border) & (y <= h - 1 - border)
    x, y, u, v, W, q = x[on], y[on], u[on], v[on], W[on], Q[on]
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    fx, fy = u - x0, v - y0
    p00, p01, p10, p11 = T[y0, x0], T[y0, x0 + 1], T[y0 + 1, x0], T[y0 + 1, x0 + 1]
    top, bot = p00 + fx * (p01 - p00), p10 + fx * (p11 - p10)
    t = top + fy * (bot - top)
    gx, gy = (p01 - p00) + fy * ((p11 - p10) - (p01 - p00)), (p10 - p00) + fx * ((p11 - p01) - (p10 - p00))
    xn, yn, un, vn = (x - cx) * s, (y - cy) * s, (u - cx) * s, (v - cy) * s
    A, B = a * gx / s / W, a * gy / s / W
    D = -(A * un + B * vn)
    cols = np.stack([A * xn, A * yn, A, B * xn, B * yn, B, D * xn, D * yn, D, t, np.ones_like(t), q - (a * t + b)], axis=1)
    return cols.T @ cols, int(on.sum())


def gauss_newton64(Q, T, H, rounds=8, border=2, min_pixels=256, damping=0.0):
    """The rounds of align_math.h in float64 -> (H [9], gain, bias, rms0, rms, accepted rounds)."""
    (h, w), (cx, cy, s) = Q.shape, norm(*Q.shape[::-1])
    N = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    cur = acc = (np.asarray(H, np.float64).reshape(9), 1.0, 0.0)
    q_acc = q0 = 0.0
    done = 0
    for k in range(rounds + 1):
        G, n = gram64(Q, T, *cur, border=border)
        if n < max(min_pixels, 1) or not np.isfinite(G).all():
            break
        q = G[11, 11] / n
        if k == 0:
            q0 = q
        elif q > q_acc:
            break
        else:
            done += 1
        acc, q_acc = cur, q
        if k == rounds:
            break
        Hn = (N @ cur[0].reshape(3, 3) @ np.linalg.inv(N)).reshape(9)
        keep = [c for c in range(11) if c != int(np.argmax(np.abs(Hn)))]
        M = G[np.ix_(keep, keep)] + damping * np.diag(np.diag(G)[keep])
        step = np.linalg.solve(M, G[keep, 11])
        Hn[keep[:8]] += step[:8]
        Hd = np.linalg.inv(N) @ Hn.reshape(3, 3) @ N
        cur = ((Hd / Hd.reshape(9)[np.argmax(np.abs(Hd))]).reshape(9), cur[1] + step[8], cur[2] + step[9])
    return acc + (math.sqrt(q0), math.sqrt(q_acc), done)


def corner_error(H, H_true, w, h):
    """The largest distance between the frame's corners under H and under H_true, in pixels."""
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], np.float64).T
    a, b = (np.asarray(m, np.float64).reshape(3, 3) @ c for m in (H, H_true))
    return float(np.hypot(*(a[:2] / a[2] - b[:2] / b[2])).max())


# ---- the analytic fixture: Q = I on the lattice, T = 0.8 I(G .) + 10, so H_true = G^-1, gain 1.25, bias -12.5 ----
W, H = 256, 192
G_TRUE = np.array([[1.02, 0.015, -6.0], [-0.02, 0.99, 5.0], [2e-5, -1e-5, 1.0]])
H_TRUE = np.linalg.inv(G_TRUE) / np.linalg.inv(G_TRUE)[2, 2]
# the start: H_TRUE with a shift, a small rotation and a perspective term - the frame's corners move by about one pixel
H_START = (np.array([[1, 0.003, 0.4], [-0.003, 1, -0.5], [1e-6, 0, 1]]) @ H_TRUE).astype(np.float32).reshape(9)


def analytic(x, y):
    """A dozen sinusoids with periods of 20 to 90 pixels around 128: smooth enough for the bilinear patch."""
    rng = np.random.default_rng(7)
    out = np.full(np.broadcast(x, y).shape, 128.0)
    for _ in range(12):
        period, angle, phase = rng.uniform(20, 90), rng.uniform(0, math.pi), rng.uniform(0, 2 * math.pi)
        out += 9.0 * np.sin(2 * math.pi / period * (math.cos(angle) * x + math.sin(angle) * y) + phase)
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    """imgs [2, 192, 256] float32: the query frame and the train frame, each sampled exactly."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y, Wd = (G_TRUE[r, 0] * x + G_TRUE[r, 1] * y + G_TRUE[r, 2] for r in range(3))
    return np.stack([analytic(x, y), 0.8 * analytic(X / Wd, Y / Wd) + 10]).astype(np.float32)
