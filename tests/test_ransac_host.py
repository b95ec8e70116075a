"""The definition of the geometric verification (sift_amd/csrc/ransac_math.h) through its host build (libsift_hostmath.so):
the sampler, the four-point solver, the predicate and the whole loop.  No GPU; tests/test_ransac_gpu.py holds the kernels to
this loop bit for bit."""
import numpy as np
import pytest

import ransac_ref as R

SQUARE = np.array([[0, 0], [1000, 0], [1000, 1000], [0, 1000]], np.float64)
MAPS = {
    "identity": np.eye(3),
    "translation": np.array([[1, 0, 37.0], [0, 1, -50.0], [0, 0, 1]]),
    "similarity": np.array([[1.2 * np.cos(0.3), -1.2 * np.sin(0.3), 900.0], [1.2 * np.sin(0.3), 1.2 * np.cos(0.3), 40.0], [0, 0, 1]]),
    "projective": np.array([[1.2, 0.3, 500.0], [-0.4, 0.9, 1900.0], [6e-4, -4e-4, 1.0]]),
}
ORIGINS = [(0, 0), (100, 100), (3096, 0), (3096, 3096), (517, 2041)]   # query coordinates up to 4096


@pytest.mark.parametrize("m", [4, 5, 6, 7, 64, 65, 1000, 70000])
def test_draw_distinct_in_range(m):
    d = R.draws(3, 1, 4096, m)
    assert d.max() < m
    assert (np.sort(d, axis=1)[:, 1:] != np.sort(d, axis=1)[:, :-1]).all()
    if m == 4:
        assert (np.sort(d, axis=1) == np.arange(4)).all()
        assert len(set(map(tuple, d.tolist()))) == 24


def test_draw_uniform_m8():
    """4096 draws of 4 out of 8: every index is expected 2048 times, standard deviation about 32 - a sanity bound."""
    n = np.bincount(R.draws(0, 0, 4096, 8).ravel(), minlength=8)
    assert n.sum() == 4 * 4096 and n.min() >= 1536 and n.max() <= 2560, n


def test_draw_depends_on_seed_set_iteration():
    base = R.draws(0, 0, 256, 1000)
    assert not (base == R.draws(1, 0, 256, 1000)).all(axis=1).any()
    assert not (base == R.draws(0, 1, 256, 1000)).all(axis=1).any()
    assert len(set(map(tuple, base.tolist()))) == 256                      # iterations differ from each other
    assert R.same_bits(base, R.draws(0, 0, 256, 1000))                      # and nothing else enters


def _solve8(q, t):
    """float64 solution of the 8 x 8 system (h8 = 1), as a 3 x 3 matrix."""
    A, b = [], []
    for (x, y), (u, v) in zip(q, t):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y])
        b += [u, v]
    return np.append(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)), 1.0).reshape(3, 3)


def _samples():
    for name, H in MAPS.items():
        for ox, oy in ORIGINS:
            q = SQUARE + (ox, oy)
            rows = np.concatenate([q, R.apply_h(H, q)], axis=1).astype(np.float32)   # the solver sees the rounded coordinates
            yield name, rows


def test_solver_own_sample_and_float64():
    """Every sample's four correspondences are inliers of its model at 0.5 px (float evaluation error at these magnitudes is
    about 1e-3 px), and the model equals numpy's float64 solution of the 8 x 8 system, both divided by their entry of largest
    magnitude.  Measured largest deviation over the set: 1.16e-8 of the largest entry (the rounding of the nine results to
    float, 2^-24 = 6.0e-8 at most for entries near 1; the double arithmetic in front of it does not show).  The bound is 8 x that
    and never below 2^-22 = 2.4e-7, so 2^-22 it is."""
    worst = 0.0
    for name, rows in _samples():
        ok, h = R.homography4(rows)
        assert ok, name
        assert all(R.inlier(h, r, 0.5) for r in rows), name
        want = _solve8(rows[:, :2].astype(np.float64), rows[:, 2:].astype(np.float64))
        want = want / want.ravel()[np.argmax(np.abs(want))]
        got = h.astype(np.float64).reshape(3, 3)
        got = got / got.ravel()[np.argmax(np.abs(got))]
        assert np.abs(h).max() == 1.0                   # the largest entry is exactly +-1
        assert float(h[6] * rows[0, 0] + h[7] * rows[0, 1] + h[8]) > 0
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest deviation from the float64 8x8 solution: {worst:.3e}")
    assert worst <= max(8 * 1.16e-8, 2.0 ** -22)


def test_solver_rejects():
    sq = np.concatenate([SQUARE, SQUARE + 5], axis=1)
    assert R.homography4(sq)[0]
    collinear = sq.copy()
    collinear[:3, :2] = [[0, 0], [10, 10], [500, 500]]
    assert not R.homography4(collinear)[0]
    collinear_t = sq.copy()
    collinear_t[1:, 2:] = [[3, 9], [6, 18], [9, 27]]
    assert not R.homography4(collinear_t)[0]
    coincident = sq.copy()
    coincident[3] = coincident[1]
    assert not R.homography4(coincident)[0]
    bowtie = sq.copy()                                     # a convex quadrilateral onto a bow-tie: two targets swapped
    bowtie[[2, 3], 2:] = bowtie[[3, 2], 2:]
    assert not R.homography4(bowtie)[0]
    mirrored = sq.copy()                                   # a reflection keeps W's sign: a legitimate model
    mirrored[:, 2] = 2000 - mirrored[:, 2]
    assert R.homography4(mirrored)[0]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            broken = sq.copy()
            broken[2, k] = bad
            ok, h = R.homography4(broken)
            assert not ok and h.tobytes() == np.zeros(9, np.float32).tobytes()


def test_predicate_nan_inf():
    h = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    assert R.inlier(h, [5, 5, 5, 8], 3.0) and not R.inlier(h, [5, 5, 5, 8.01], 3.0)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            row = [5.0, 5.0, 5.0, 5.0]
            row[k] = bad
            assert not R.inlier(h, row, 3.0)
    grow = np.array([1, 0, 0, 0, 1, 0, 1, 0, 1], np.float32)   # W grows with qx: an infinite qx gives inf <= inf, which is no inlier
    assert not R.inlier(grow, [np.inf, 0, -1, -1], 3.0)
    assert not R.inlier(-h, [5, 5, 5, 5], 3.0)                   # W < 0


def test_whole_300():
    """300 correspondences under a projective map, 60 % replaced by uniform random targets; 512 iterations, 3 px, seed 0.
    (The host loop met the conditions below for this seed - and for seeds 1 .. 7 - before the seed was fixed.)"""
    rows, err = R.projective_rows(np.random.default_rng(0), 300)
    models, flags, scores = R.ransac(rows, None, 512, 3.0, 0)
    true_in = err < 0.01
    assert 80 < true_in.sum() < 160
    assert flags[true_in].all()
    assert not flags[err > 50].any()
    m = models[0]
    assert m["iteration"] == int(np.argmax(scores[0]))                 # the first maximum
    assert m["inliers"] == flags.sum() == scores[0, m["iteration"]]
    assert (scores >= -1).all() and (scores == -1).any()               # degenerate and orientation-flipping samples
    corners = np.array([[0, 0], [999, 0], [999, 999], [0, 999]], np.float64)
    assert np.abs(R.apply_h(m["h"], corners) - R.apply_h(R.H_PROJ, corners)).max() < 3.0


@pytest.mark.parametrize("case", ["m0", "m1", "m3", "collinear", "identical"])
def test_degenerate_sets(case):
    rng = np.random.default_rng(2)
    rows = {"m0": R.random_rows(rng, 0), "m1": R.random_rows(rng, 1), "m3": R.random_rows(rng, 3),
            "collinear": np.stack([np.arange(40.0), 2 * np.arange(40.0) + 1, np.arange(40.0) + 3, 2 * np.arange(40.0)], axis=1),
            "identical": np.full((40, 4), 17.0)}[case]
    models, flags, scores = R.ransac(rows, None, 64, 3.0, 0)
    assert models[0]["iteration"] == -1 and models[0]["inliers"] == 0
    assert models[0]["h"].tobytes() == np.zeros(9, np.float32).tobytes()
    assert not flags.any() and (scores == -1).all()


def test_many_sets_use_their_set_number():
    """Set s of a call draws with set number s: the same rows at another position give another sequence, the same position the
    same result."""
    rng = np.random.default_rng(5)
    a, _ = R.projective_rows(rng, 80)
    b = R.random_rows(rng, 33)
    both = np.concatenate([a, b, a])
    models, flags, scores = R.ransac(both, [0, 80, 113, 193], 128, 3.0, 9)
    alone = R.ransac(a, None, 128, 3.0, 9)
    assert R.same_bits(scores[0], alone[2][0]) and R.same_bits(models[:1], alone[0]) and R.same_bits(flags[:80], alone[1])
    assert not R.same_bits(scores[2], scores[0])
    # a set in front that is empty moves the set number, not the rows
    shifted = R.ransac(np.concatenate([a, b]), [0, 0, 80, 113], 128, 3.0, 9)
    assert not R.same_bits(shifted[2][1], scores[0]) and shifted[0][0]["iteration"] == -1
