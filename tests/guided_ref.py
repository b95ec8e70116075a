"""Shared by tests/test_guided_host.py and tests/test_guided_gpu.py: the host checker of guided matching
(hostmath_match_knn2_guided in libsift_hostmath.so: the definition of include/sift_hip.h, "guided matching", as plain loops over
the two verification predicates), a numpy restatement of that definition that shares no code with it, and the generators."""
import ctypes as C

import numpy as np

import fund_ref as F
import match_ref as M
import ransac_ref as R

ROOT = M.ROOT
same_bits = M.same_bits
KINDS = {"homography": 0, "fundamental": 1}
_bound = False


def hostmath():
    global _bound
    H = M.hostmath()
    if not _bound:
        vp, ll = C.c_void_p, C.c_longlong
        H.hostmath_match_knn2_guided.argtypes = [vp, vp, vp, ll, vp, vp, vp, ll, C.c_int, vp, C.c_float, C.c_int, vp, vp]
        H.hostmath_match_knn2_guided.restype = None
        _bound = True
    return H


def _f32(a, shape):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def knn2(q, t, q_xy, t_xy, kind, model, threshold, q_valid=None, t_valid=None, reverse=False):
    """(idx, dist2) by the checker: [nq, 2] the top-2 admissible train rows of every query row, or with `reverse` [nt, 2] the
    top-2 query rows of every train row under the same predicate (the cross-check's reverse best)."""
    q, t = _f32(q, (-1, 128)), _f32(t, (-1, 128))
    q_xy, t_xy, model = _f32(q_xy, (-1, 2)), _f32(t_xy, (-1, 2)), _f32(model, 9)
    assert q_xy.shape[0] == q.shape[0] and t_xy.shape[0] == t.shape[0]
    qv = None if q_valid is None else np.ascontiguousarray(q_valid, np.uint8)
    tv = None if t_valid is None else np.ascontiguousarray(t_valid, np.uint8)
    n = t.shape[0] if reverse else q.shape[0]
    idx = np.zeros((n, 2), np.int32)
    dist = np.zeros((n, 2), np.float32)
    hostmath().hostmath_match_knn2_guided(q.ctypes.data, None if qv is None else qv.ctypes.data, q_xy.ctypes.data, q.shape[0], t.ctypes.data,
                                          None if tv is None else tv.ctypes.data, t_xy.ctypes.data, t.shape[0], KINDS[kind],
                                          model.ctypes.data, threshold, 1 if reverse else 0, idx.ctypes.data, dist.ctypes.data)
    return idx, dist


def matches(q, t, q_xy, t_xy, kind, model, threshold, ratio, cross_check, q_valid=None, t_valid=None):
    """The records sift_hip_match_guided must deliver for one pair, from the checker."""
    fwd = knn2(q, t, q_xy, t_xy, kind, model, threshold, q_valid, t_valid)
    rev = knn2(q, t, q_xy, t_xy, kind, model, threshold, q_valid, t_valid, reverse=True)
    return M.filter_matches(fwd[0], fwd[1], ratio, cross_check, rev[0])


# ---- the numpy restatement: float32, every rounding where the definition has one ------------------------------
def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product of two floats is exact in double; the double sum is rounded to odd (its
    rounding error by TwoSum), after which the rounding to float cannot be a double rounding (53 >= 2 * 24 + 2)."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
        c = np.asarray(c, np.float32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def d2_matrix(q, t):
    """d2 of every (query, train) as the header's chain: [nq, nt] float32."""
    q, t = _f32(q, (-1, 128)), _f32(t, (-1, 128))

    def dots(a, b):   # a [n, 1, 128] against b [1, m, 128]
        acc = np.zeros(np.broadcast_shapes(a.shape[:2], b.shape[:2]), np.float32)
        for k in range(128):
            acc = fma32(a[..., k], b[..., k], acc)
        return acc
    with np.errstate(all="ignore"):
        nq, nt = dots(q[:, None], q[:, None]), dots(t[None], t[None])
        v = (nq + nt) - np.float32(2) * dots(q[:, None], t[None])
        return np.where(v < 0, np.float32(0), v).astype(np.float32)


def admissible(kind, model, q_xy, t_xy, threshold):
    """[nq, nt] bool: the predicate of ransac_math.h / ransac_fund_math.h, operation for operation, in float32."""
    m = _f32(model, 9)
    qx, qy = _f32(q_xy, (-1, 2))[:, 0][:, None], _f32(q_xy, (-1, 2))[:, 1][:, None]
    tx, ty = _f32(t_xy, (-1, 2))[:, 0][None], _f32(t_xy, (-1, 2))[:, 1][None]
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        thr2 = np.float32(threshold) * np.float32(threshold)   # may overflow to +inf
        if kind == "homography":
            X = fma32(m[0], qx, fma32(m[1], qy, m[2]))
            Y = fma32(m[3], qx, fma32(m[4], qy, m[5]))
            W = fma32(m[6], qx, fma32(m[7], qy, m[8]))
            ex, ey = fma32(-tx, W, X), fma32(-ty, W, Y)
            e2 = fma32(ex, ex, ey * ey)
            return (W > 0) & (e2 <= thr2 * (W * W)) & (e2 < inf)
        a = fma32(m[0], qx, fma32(m[1], qy, m[2]))
        b = fma32(m[3], qx, fma32(m[4], qy, m[5]))
        c = fma32(m[6], qx, fma32(m[7], qy, m[8]))
        r = fma32(tx, a, fma32(ty, b, c))
        a2 = fma32(m[0], tx, fma32(m[3], ty, m[6]))
        b2 = fma32(m[1], tx, fma32(m[4], ty, m[7]))
        g = fma32(a, a, fma32(b, b, fma32(a2, a2, b2 * b2)))
        e = r * r
        return (e <= thr2 * g) & (g > 0) & (e < inf)


def top2(d, cand):
    """The first two candidates of every row of d [n, m] in the order (d, column): (idx [n, 2], dist [n, 2])."""
    n, m = d.shape
    idx = np.full((n, 2), -1, np.int32)
    dist = np.full((n, 2), np.inf, np.float32)
    if m == 0:
        return idx, dist
    key = np.where(cand, d, np.float32(np.inf))
    order = np.argsort(key, axis=1, kind="stable")
    order = np.take_along_axis(order, np.argsort(~np.take_along_axis(cand, order, axis=1), axis=1, kind="stable"), axis=1)
    count = cand.sum(axis=1)
    for k in range(min(2, m)):
        has = count > k
        idx[has, k] = order[has, k]
        dist[has, k] = d[has, order[has, k]]
    return idx, dist


def knn2_numpy(q, t, q_xy, t_xy, kind, model, threshold, q_valid=None, t_valid=None, reverse=False):
    d = d2_matrix(q, t)
    qv = np.ones(d.shape[0], bool) if q_valid is None else np.asarray(q_valid) != 0
    tv = np.ones(d.shape[1], bool) if t_valid is None else np.asarray(t_valid) != 0
    cand = admissible(kind, model, q_xy, t_xy, threshold) & qv[:, None] & tv[None] & ~np.isnan(d)
    return top2(d.T, cand.T) if reverse else top2(d, cand)


# ---- generators -------------------------------------------------------------------------------------------------
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
# g > 0 at every finite row: a = 1, b = 0 whatever the points are
F_ADMIT_ALL = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)


def banded_scene(rng, nq, nt, kind, size=1000.0):
    """Points and a model under which a band of `threshold` pixels admits roughly a tenth of the train rows for a query row:
    -> (q_xy, t_xy, model [9], threshold).  Homography: the query points fill a square of 60 px, the train points its image; a
    disc of 12 px is an eighth of that, less at the edges.  Fundamental: the points are spread over the image and the band
    around a line covers about a tenth of it."""
    q_xy = np.floor(rng.random((nq, 2)) * size).astype(np.float32)
    if kind == "homography":
        model = (R.H_PROJ / np.abs(R.H_PROJ).max()).astype(np.float32).ravel()
        q_xy = np.floor(400.0 + rng.random((nq, 2)) * 60.0).astype(np.float32)
        t_xy = R.apply_h(model.astype(np.float64), 400.0 + rng.random((nt, 2)) * 60.0).astype(np.float32)
        return q_xy, t_xy, model, 12.0
    _, _, Fm = F.two_view_scene(rng)
    t_xy = (rng.random((nt, 2)) * F.SIZE).astype(np.float32)
    q_xy = (q_xy * np.float32(F.SIZE / size)).astype(np.float32)
    return q_xy, t_xy, Fm.astype(np.float32).ravel(), 100.0


def twin_scene(seed, kind, n=400, twins=200, noise=0.01):
    """n true pairs under a model; query rows 0 .. twins - 1 each have a twin in the train set, a second noisy copy of the same
    descriptor 50 to 300 px off the true target (for the fundamental matrix: along the normal of the row's epipolar line).
    The train order is permuted -> (q, t, q_xy, t_xy, model [9] float32, truth [n]: the train row of every query row,
    twin_of [twins]: the train row of every twin)."""
    rng = np.random.default_rng(seed)
    base = M.desc_rows(rng, n)
    if kind == "homography":
        model = R.H_PROJ
        q_xy = rng.uniform(100.0, 1900.0, (n, 2))
        target = R.apply_h(model, q_xy)
        ang = rng.uniform(0, 2 * np.pi, twins)
        normal = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    else:
        rows, model, _ = F.two_view_rows(rng, n)
        q_xy, target = rows[:, :2].astype(np.float64), rows[:, 2:].astype(np.float64)
        line = np.concatenate([q_xy[:twins], np.ones((twins, 1))], axis=1) @ np.asarray(model).reshape(3, 3).T
        normal = line[:, :2] / np.hypot(line[:, 0], line[:, 1])[:, None] * rng.choice([-1.0, 1.0], twins)[:, None]
    off = target[:twins] + normal * rng.uniform(50.0, 300.0, twins)[:, None]

    def noisy(d):
        return (d + noise * rng.standard_normal(d.shape)).astype(np.float32)
    q = noisy(base)
    t = np.concatenate([noisy(base), noisy(base[:twins])])
    t_xy = np.concatenate([target, off])
    perm = rng.permutation(n + twins)
    where = np.argsort(perm)                     # old row -> new row
    return (q, np.ascontiguousarray(t[perm]), q_xy.astype(np.float32), np.ascontiguousarray(t_xy[perm].astype(np.float32)),
            np.asarray(model, np.float32).ravel(), where[:n], where[n:])


def ratio_keep(idx, dist, ratio):
    r2 = np.float32(ratio) * np.float32(ratio)
    with np.errstate(invalid="ignore"):
        return (idx[:, 0] >= 0) & (dist[:, 0] < (r2 * dist[:, 1]).astype(np.float32))
