"""Shared by tests/test_fundamental_host.py and tests/test_fundamental_gpu.py: the host checker of the epipolar verification
(hostmath_ransac_fundamental and its pieces in libsift_hostmath.so: sift_amd/csrc/ransac_fund_math.h in plain loops) and the
generators of two-view correspondences."""
import ctypes as C

import numpy as np

import ransac_ref as R

ROOT = R.ROOT
same_bits = R.same_bits
MODEL_DTYPE = np.dtype([("f", "<f4", (9,)), ("inliers", "<i4"), ("iteration", "<i4"), ("root", "<i4")])
assert MODEL_DTYPE.itemsize == 48
_bound = False


def hostmath():
    global _bound
    H = R.hostmath()
    if not _bound:
        vp, u32 = C.c_void_p, C.c_uint32
        H.hostmath_ransac_draw7.argtypes = [u32, u32, u32, u32, vp]
        H.hostmath_ransac_draw7.restype = None
        H.hostmath_fundamental7.argtypes = [vp, vp]
        H.hostmath_fund_inlier.argtypes = [vp, vp, C.c_float]
        H.hostmath_ransac_fundamental.argtypes = [vp, C.c_int, vp, u32, u32, C.c_float, vp, vp, vp]
        H.hostmath_ransac_fundamental.restype = None
        _bound = True
    return H


def draw7(seed, set_, iteration, m):
    idx = np.zeros(7, np.uint32)
    hostmath().hostmath_ransac_draw7(seed, set_, iteration, m, idx.ctypes.data)
    return idx


def fundamental7(rows):
    """(valid [3] bool, f [3, 9] float32) of seven correspondences (qx, qy, tx, ty)."""
    c = np.ascontiguousarray(rows, np.float32).reshape(7, 4)
    f = np.full((3, 9), 7, np.float32)
    mask = hostmath().hostmath_fundamental7(c.ctypes.data, f.ctypes.data)
    return np.array([(mask >> k) & 1 for k in range(3)], bool), f


def inlier(f, row, thr):
    f = np.ascontiguousarray(f, np.float32)
    row = np.ascontiguousarray(row, np.float32)
    return bool(hostmath().hostmath_fund_inlier(f.ctypes.data, row.ctypes.data, thr))


def ransac(pts, offsets=None, iterations=2048, threshold=1.0, seed=0):
    """(models [n_sets] MODEL_DTYPE, inlier [rows] uint8, scores [n_sets, 3 * iterations] int32) by the checker."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    offsets = np.array([0, pts.shape[0]], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64)
    n = offsets.size - 1
    models = np.zeros(n, MODEL_DTYPE)
    flags = np.zeros(pts.shape[0], np.uint8)
    scores = np.zeros((n, 3 * iterations), np.int32)
    hostmath().hostmath_ransac_fundamental(pts.ctypes.data, n, offsets.ctypes.data, iterations, seed, threshold, models.ctypes.data,
                                           flags.ctypes.data, scores.ctypes.data)
    return models, flags, scores


SIZE, FOCAL = 2048.0, 1500.0


def _rotation(w):
    """Rodrigues: the rotation about the axis w by |w| radians."""
    t = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def two_view_scene(rng):
    """A well-conditioned pair of cameras, focal length 1500, principal point at the centre of a 2048-pixel image: a rotation of
    a few degrees and a baseline of about one tenth of the scene depth -> (P1, P2 [3, 4], F [3, 3] with t^T F q = 0)."""
    K = np.array([[FOCAL, 0, SIZE / 2], [0, FOCAL, SIZE / 2], [0, 0, 1]])
    Rm = _rotation(rng.uniform(-0.1, 0.1, 3) + 1e-3)
    t = rng.uniform(-1.0, 1.0, 3) * [0.5, 0.5, 0.2] + [1.5, 0.0, 0.0]   # sideways: both epipoles are far outside the images
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ Rm @ Ki
    return K @ np.eye(3, 4), K @ np.concatenate([Rm, t[:, None]], axis=1), F / np.abs(F).max()


def two_view_rows(rng, m, scene=None, outliers=0.0):
    """m correspondences of random 3-D points (depth 6 .. 20) seen by both cameras inside the image, float32 rows; a share of
    them with uniform random targets -> (rows, F, distance of every row's target from its true epipolar line in pixels)."""
    P1, P2, F = two_view_scene(rng) if scene is None else scene
    rows = np.zeros((0, 4))
    while rows.shape[0] < m:
        z = rng.uniform(6.0, 20.0, 4 * m)
        X = np.stack([rng.uniform(-0.7, 0.7, 4 * m) * z, rng.uniform(-0.7, 0.7, 4 * m) * z, z, np.ones(4 * m)])
        a, b = P1 @ X, P2 @ X
        cand = np.concatenate([a[:2] / a[2], b[:2] / b[2]]).T
        keep = (cand.min(axis=1) >= 0) & (cand.max(axis=1) <= SIZE) & (b[2] > 0)
        rows = np.concatenate([rows, cand[keep]])
    rows = rows[:m]
    bad = rng.random(m) < outliers
    rows[bad, 2:] = rng.random((int(bad.sum()), 2)) * SIZE
    rows = np.ascontiguousarray(rows, np.float32)
    return rows, F, epipolar_distance(F, rows)


def epipolar_distance(F, rows):
    """float64 distance in pixels of every target (tx, ty) from the line F (qx, qy, 1)."""
    rows = np.asarray(rows, np.float64)
    q = np.concatenate([rows[:, :2], np.ones((len(rows), 1))], axis=1)
    t = np.concatenate([rows[:, 2:], np.ones((len(rows), 1))], axis=1)
    line = q @ np.asarray(F, np.float64).reshape(3, 3).T
    return np.abs((line * t).sum(axis=1)) / np.hypot(line[:, 0], line[:, 1])


def fixed_samples(n=48):
    """The fixed list of seven-point samples of the solver tests: sample i comes from a two-view scene of its own, rng seed
    1000 + i (two_view_scene: a sideways baseline, so both epipoles lie far outside the images)."""
    return [two_view_rows(np.random.default_rng(1000 + i), 7)[0] for i in range(n)]


def random_rows(rng, m):
    return np.ascontiguousarray(rng.random((m, 4)) * SIZE, np.float32)


def numpy_models(rows):
    """The seven-point models of float32 rows by an independent float64 route: the SVD null space of the 7 x 9 matrix, np.roots on
    the cubic det(l n1 + n2) (coefficients by exact interpolation of a cubic at four points), the real roots -> [k, 9], each
    divided by its entry of largest magnitude."""
    r = np.asarray(rows, np.float64).reshape(7, 4)
    qx, qy, tx, ty = r.T
    A = np.stack([tx * qx, tx * qy, tx, ty * qx, ty * qy, ty, qx, qy, np.ones(7)], axis=1)
    vt = np.linalg.svd(A)[2]
    n1, n2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    coef = np.linalg.solve(np.vander(xs, 4), [np.linalg.det(x * n1 + n2) for x in xs])
    out = []
    for z in np.roots(coef):
        if abs(z.imag) <= 1e-9 * max(1.0, abs(z)):
            F = (z.real * n1 + n2).ravel()
            out.append(F / F[np.argmax(np.abs(F))])
    return np.array(out).reshape(-1, 9)
