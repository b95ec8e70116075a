"""Shared by tests/test_fund_refine_host.py and tests/test_fund_refine_gpu.py: the host checker of the refit of F
(hostmath_refine_fundamental and hostmath_fund_refine_sums in libsift_hostmath.so: sift_amd/csrc/ransac_fund_refine_math.h in
plain loops), a float64 numpy restatement of one round, and the noisy two-view sets with their starting models."""
import ctypes as C

import numpy as np

import fund_ref as FR

MODEL_DTYPE = FR.MODEL_DTYPE
_bound = False


def hostmath():
    global _bound
    H = FR.hostmath()
    if not _bound:
        vp = C.c_void_p
        H.hostmath_refine_fundamental.argtypes = [vp, C.c_int, vp, C.c_float, C.c_int, vp, vp, vp]
        H.hostmath_refine_fundamental.restype = None
        H.hostmath_fund_refine_sums.argtypes = [vp, C.c_longlong, vp, C.c_float, vp, vp]
        _bound = True
    return H


def model_of(F, iteration=0, root=0):
    """One MODEL_DTYPE record holding F divided by its first entry of largest magnitude, as a caller-supplied model."""
    F = np.asarray(F, np.float64).ravel()
    m = np.zeros(1, MODEL_DTYPE)
    m["f"][0] = (F / F[np.argmax(np.abs(F))]).astype(np.float32)
    m["iteration"], m["root"], m["inliers"] = iteration, root, -5   # inliers: ignored and rewritten
    return m


def refine(pts, models, offsets=None, threshold=3.0, rounds=8):
    """(models, refined [n_sets] int32, inlier [rows] uint8) of hostmath_refine_fundamental from the given models (copied)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    offsets = np.array([0, pts.shape[0]], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
    models = np.array(models, MODEL_DTYPE).reshape(-1)
    assert models.size == offsets.size - 1
    refined = np.full(models.size, 77, np.int32)
    flags = np.full(pts.shape[0], 7, np.uint8)
    hostmath().hostmath_refine_fundamental(pts.ctypes.data, models.size, offsets.ctypes.data, threshold, rounds, models.ctypes.data,
                                           refined.ctypes.data, flags.ctypes.data)
    return models, refined, flags


def sums(pts, f, threshold=3.0):
    """(n, sums [36] float64 with sums[0] = n, (cqx, cqy, sq, ctx, cty, st)); n = -1 - inliers when the round fails there."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    f = np.ascontiguousarray(f, np.float32)
    out, norm = np.full(36, np.nan), np.full(6, np.nan)
    n = hostmath().hostmath_fund_refine_sums(pts.ctypes.data, pts.shape[0], f.ctypes.data, threshold, out.ctypes.data, norm.ctypes.data)
    return n, out, norm


def _rank2(Fn):
    w, V = np.linalg.eigh(Fn.T @ Fn)
    v = V[:, 0]
    return Fn - np.outer(Fn @ v, v)


def numpy_round(rows, f, keep, norm):
    """One round of the recipe in float64 numpy from the model f, over the rows `keep` under the normalisation `norm`: the 9 x 9
    moment matrix S, and the new model (numpy.linalg.solve on the reduced system, eigh for the rank-2 step), its largest entry 1."""
    cqx, cqy, sq, ctx, cty, st = norm
    r = np.asarray(rows, np.float64)[keep]
    x, y, u, v = (r[:, 0] - cqx) * sq, (r[:, 1] - cqy) * sq, (r[:, 2] - ctx) * st, (r[:, 3] - cty) * st
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=1)
    S = A.T @ A
    Tq = np.array([[sq, 0, -sq * cqx], [0, sq, -sq * cqy], [0, 0, 1]])
    Tt = np.array([[st, 0, -st * ctx], [0, st, -st * cty], [0, 0, 1]])
    Fn = np.linalg.inv(Tt).T @ np.asarray(f, np.float64).reshape(3, 3) @ np.linalg.inv(Tq)
    e = int(np.argmax(np.abs(Fn)))
    k = [i for i in range(9) if i != e]
    g = np.zeros(9)
    g[e] = 1.0
    g[k] = np.linalg.solve(S[np.ix_(k, k)], -S[k, e])
    F = (Tt.T @ _rank2(g.reshape(3, 3)) @ Tq).ravel()
    return S, F / F[np.argmax(np.abs(F))]


def noisy_case(seed, m=300, noise=0.5):
    """The fixed set of `seed`: m rows of a two-view scene (coordinates 0 .. 2048), Gaussian noise on both points -> (rows
    float32, clean rows float64, the starting model: the null vector of 8 random rows, which stands in for a minimal winner)."""
    rng = np.random.default_rng(seed)
    clean = FR.two_view_rows(rng, m)[0].astype(np.float64)
    rows = (clean + rng.normal(0.0, noise, clean.shape)).astype(np.float32)
    q = rows[rng.choice(m, 8, replace=False)].astype(np.float64)
    A = np.stack([q[:, 2] * q[:, 0], q[:, 2] * q[:, 1], q[:, 2], q[:, 3] * q[:, 0], q[:, 3] * q[:, 1], q[:, 3], q[:, 0], q[:, 1], np.ones(8)], axis=1)
    start = model_of(np.linalg.svd(A)[2][-1], iteration=3, root=1)
    return rows, clean, start
