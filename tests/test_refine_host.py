"""The definition of the RANSAC refinement (sift_amd/csrc/ransac_refine_math.h) through its host build (libsift_hostmath.so):
the fixed-order sums, the 8 x 8 solve, whole rounds and what they are worth.  No GPU; tests/test_refine_gpu.py holds the kernel
to this loop bit for bit."""
from fractions import Fraction

import numpy as np
import pytest

import ransac_ref as R
import refine_ref as F

H32 = R.H_PROJ.astype(np.float32).ravel()


def _fma(a, b, c):
    """fma(a, b, c) of three doubles: the exact value, rounded once (int / int division in Python is correctly rounded)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _restated_terms(rows, nm):
    """The 6 moment terms and the 22 normal terms of every row in numpy float64, products and sums one rounding each as the
    header writes them; its one fused operation, r = fma(u, u, v * v), by exact arithmetic."""
    q = rows.astype(np.float64)
    mom = np.stack([q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1], q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]], axis=1)
    if nm is None:
        return mom, None
    cqx, cqy, sq, ctx, cty, st = nm
    x, y = (q[:, 0] - cqx) * sq, (q[:, 1] - cqy) * sq
    u, v = (q[:, 2] - ctx) * st, (q[:, 3] - cty) * st
    xx, xy, yy = x * x, x * y, y * y
    r = np.array([_fma(a, a, b * b) for a, b in zip(u, v)], np.float64).reshape(-1)
    one = np.ones_like(x)
    geo = [xx, xy, yy, x, y]
    nrm = np.stack(geo + [u * g for g in geo + [one]] + [v * g for g in geo + [one]] + [r * g for g in geo], axis=1)
    return mom, nrm


def _sum_rows(m):
    """Noisy rows with 30 % outliers; the five-row set has none, so that a round has its four inliers."""
    return R.projective_rows(np.random.default_rng(m), m, outliers=0.3 if m > 5 else 0.0, noise=0.5)[0]


@pytest.mark.parametrize("m", [5, 256, 257, 1000])
def test_summation_order(m):
    """hostmath_refine_sums against the restatement `256 strided partials, adjacent tree`, bit for bit."""
    rows = _sum_rows(m)
    keep = np.array([R.inlier(H32, r, 3.0) for r in rows])
    idx = np.nonzero(keep)[0]
    n, sums = F.refine_sums(rows, H32, 3.0)
    assert n == idx.size >= 4
    mom_terms, _ = _restated_terms(rows[idx], None)
    mom = F.fixed_order_sum(mom_terms, idx)
    assert R.same_bits(sums[:6], mom)
    ok, nm = F.normalisation(mom, n)
    assert ok
    for (sx, sy, s2, scale) in ((mom[0], mom[1], mom[4], nm[2]), (mom[2], mom[3], mom[5], nm[5])):
        d = s2 / n - ((sx / n) ** 2 + (sy / n) ** 2)
        assert np.frexp(scale)[0] == 0.5 and 0.99 <= d * scale * scale < 4.01   # a power of two that brings the spread to [1, 4)
    assert nm[0] == mom[0] / n and nm[4] == mom[3] / n
    _, nrm_terms = _restated_terms(rows[idx], nm)
    assert R.same_bits(sums[6:], F.fixed_order_sum(nrm_terms, idx))


def test_summation_order_is_told_apart():
    """A plain np.sum of the same terms differs from the fixed-order sum: the test above can tell the orders apart."""
    differs = 0
    for m in (5, 256, 257, 1000):
        rows = _sum_rows(m)
        idx = np.nonzero([R.inlier(H32, r, 3.0) for r in rows])[0]
        n, sums = F.refine_sums(rows, H32, 3.0)
        ok, nm = F.normalisation(sums[:6], n)
        _, nrm_terms = _restated_terms(rows[idx], nm)
        plain = nrm_terms.sum(axis=0)
        seq = np.zeros(22)
        for t in nrm_terms:
            seq = seq + t
        differs += int(not R.same_bits(plain, sums[6:])) + int(not R.same_bits(seq, sums[6:]))
        assert np.allclose(plain, sums[6:], rtol=1e-9, atol=1e-9)
    assert differs >= 1


def test_solve8_against_lapack():
    """50 random well-conditioned SPD systems (B B^T + 8 I, B standard normal) against numpy.linalg.solve.  Largest relative
    difference max|x - x_np| / max|x_np| measured on the CPU over these 50: 5.3e-16 (the pivot order differs from LAPACK's, so
    not 0).  The bound is 8 x that, 4.3e-15."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(50):
        B = rng.standard_normal((8, 8))
        A = B @ B.T + 8 * np.eye(8)
        b = rng.standard_normal(8)
        ok, x = F.solve8(A, b)
        assert ok
        want = np.linalg.solve(A, b)
        worst = max(worst, float(np.abs(x - want).max() / np.abs(want).max()))
    print(f"largest relative difference from numpy.linalg.solve: {worst:.3e}")
    assert worst <= 4.3e-15   # 8 x 5.3e-16, the largest difference measured


def test_solve8_pivots_and_failures():
    rng = np.random.default_rng(1)
    P = np.eye(8)[rng.permutation(8)]           # zero diagonal entries: nothing works without the row exchanges
    b = np.arange(1.0, 9.0)
    ok, x = F.solve8(P, b)
    assert ok and R.same_bits(x, P.T @ b)
    A = rng.standard_normal((8, 8))
    singular = A.copy()
    singular[:, 5] = 0.0                        # an exactly zero column: the pivot of step 5 is 0
    assert not F.solve8(singular, b)[0]
    assert not F.solve8(np.zeros((8, 8)), b)[0]
    for where in ((0, 0), (3, 6), (7, 7)):
        bad = A.copy()
        bad[where] = np.nan
        assert not F.solve8(bad, b)[0]
    assert not F.solve8(A, np.where(np.arange(8) == 2, np.inf, b))[0]
    assert F.solve8(A, b)[0]


def _perturbed_model(px=1.0):
    """The homography of the square's corners under H_PROJ with one target moved by `px` pixels."""
    t = R.apply_h(R.H_PROJ, F.CORNERS)
    t[2] += [px, 0.0]
    ok, h = R.homography4(np.concatenate([F.CORNERS, t], axis=1))
    assert ok
    return h


def test_exact_data():
    """Rows under H_PROJ without noise (targets rounded to float), 60 % outliers, from a model that is 1 px off at one corner."""
    rows, err = R.projective_rows(np.random.default_rng(3), 600, outliers=0.6, noise=0.0)
    start = _perturbed_model()
    assert 0.9 < F.corner_error(start) < 1.1
    models, flags = F.refine(rows, F.model_of(start, 5), None, 3.0, 8)
    m = models[0]
    clean = err < 0.01
    assert 200 < clean.sum() and flags[clean].all()
    assert 1 <= m["refined"] <= 8 and m["iteration"] == 5 and m["inliers"] == flags.sum()
    print(f"corner error {F.corner_error(start):.4f} -> {F.corner_error(m['h']):.6f} px in {m['refined']} rounds")
    assert F.corner_error(m["h"]) < 0.01
    assert np.abs(m["h"]).max() == 1.0 and m["h"][6] * 500 + m["h"][7] * 500 + m["h"][8] > 0


def test_quality_20_seeds():
    """600 rows, 60 % outliers, 0.5 px noise, 512 hypotheses, 3 px, refine 8, seeds 0 .. 19: the refined model's largest corner
    error on the 1000 px square is below the minimal-sample model's in at least 18 seeds, and at most 1.0 px in all 20."""
    better, worst, report = 0, 0.0, []
    for seed in range(20):
        rows, _ = R.projective_rows(np.random.default_rng(seed), 600, outliers=0.6, noise=0.5)
        base = R.ransac(rows, None, 512, 3.0, seed)[0][0]
        fine = F.ransac(rows, None, 512, 3.0, seed, refine=8)[0][0]
        e0, e1 = F.corner_error(base["h"]), F.corner_error(fine["h"])
        report.append(f"seed {seed}: {e0:.3f} -> {e1:.3f} px, inliers {base['inliers']} -> {fine['inliers']}, {fine['refined']} rounds")
        better += int(e1 < e0)
        worst = max(worst, e1)
    print("\n".join(report))
    assert better >= 18, report
    assert worst <= 1.0, report


def _many_sets(n_sets, seed):
    rng = np.random.default_rng(seed)
    parts, sizes = [], []
    for s in range(n_sets):
        m = int(rng.integers(0, 90)) if s % 5 else int(rng.integers(200, 700))
        parts.append(R.random_rows(rng, m) if s % 2 else R.projective_rows(rng, m, outliers=0.5, noise=0.5)[0])
        sizes.append(m)
    return np.concatenate(parts).reshape(-1, 4), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_properties_200_sets():
    pts, off = _many_sets(200, 11)
    old = R.ransac(pts, off, 128, 3.0, 4)
    zero = F.ransac(pts, off, 128, 3.0, 4, refine=0)
    assert zero[0].tobytes() == old[0].tobytes() and R.same_bits(zero[1], old[1]) and R.same_bits(zero[2], old[2])
    accepted = 0
    for refine in (1, 3, 8):
        models, flags, scores = F.ransac(pts, off, 128, 3.0, 4, refine=refine)
        assert (models["inliers"] >= old[0]["inliers"]).all()
        assert (models["refined"] >= 0).all() and (models["refined"] <= refine).all()
        assert R.same_bits(models["iteration"], old[0]["iteration"]) and R.same_bits(scores, old[2])
        assert (models["inliers"] == np.add.reduceat(np.append(flags, 0).astype(np.int64), off[:-1]) * (np.diff(off) > 0)).all()
        none = models["iteration"] < 0
        assert none.any() and models[none].tobytes() == old[0][none].tobytes()
        untouched = models["refined"] == 0
        assert R.same_bits(models["h"][untouched], old[0]["h"][untouched])
        accepted += int(models["refined"].sum())
        # the separate entry from the minimal-sample models: the same result
        again, again_flags = F.refine(pts, old[0].view(F.MODEL_DTYPE), off, 3.0, refine)
        assert again.tobytes() == models.tobytes() and R.same_bits(again_flags, flags)
    assert accepted > 100


def test_collinear_inliers_leave_the_model():
    """Every inlier on one horizontal line: the normalised y is exactly 0, a pivot is exactly 0, the round fails."""
    rng = np.random.default_rng(6)
    q = np.stack([np.floor(rng.random(40) * 1000), np.full(40, 300.0)], axis=1)
    line = np.concatenate([q, q + [5.0, 7.0]], axis=1)
    rows = np.concatenate([line, R.random_rows(rng, 60)]).astype(np.float32)[rng.permutation(100)]
    start = F.model_of([[1, 0, 5], [0, 1, 7], [0, 0, 1]], 3)
    models, flags = F.refine(rows, start, None, 3.0, 8)
    assert models[0]["refined"] == 0 and R.same_bits(models[0]["h"], start[0]["h"]) and models[0]["iteration"] == 3
    assert 40 <= models[0]["inliers"] == flags.sum() <= 45


@pytest.mark.parametrize("m", [0, 1, 3])
def test_small_sets(m):
    rows = R.projective_rows(np.random.default_rng(m), m, outliers=0.0)[0]
    models, flags, _ = F.ransac(rows, None, 64, 3.0, 0, refine=8)
    assert models[0]["iteration"] == -1 and models[0]["inliers"] == 0 and models[0]["refined"] == 0 and not flags.any()
    # a caller's model over such a set is counted, not refined; a model that is none is left alone
    given, gflags = F.refine(rows, F.model_of(R.H_PROJ), None, 3.0, 8)
    assert given[0]["refined"] == 0 and given[0]["inliers"] == m == gflags.sum() and R.same_bits(given[0]["h"], H32)
    none = F.model_of(R.H_PROJ, -1)
    left, lflags = F.refine(rows, none, None, 3.0, 8)
    assert left.tobytes() == none.tobytes() and not lflags.any()


def test_nan_and_infinity_take_no_part():
    rows, _ = R.projective_rows(np.random.default_rng(9), 400, outliers=0.5, noise=0.5)
    bad = rows.copy()
    spoiled = [3, 77, 130, 131, 399]
    keep = np.ones(400, bool)
    keep[spoiled] = False
    bad[3, 0] = np.nan
    bad[77, 3] = np.inf
    bad[130, 1] = -np.inf
    bad[131] = np.nan
    bad[399, 2] = np.inf
    start = F.model_of(_perturbed_model(2.0))
    models, flags = F.refine(bad, start, None, 3.0, 8)
    assert models[0]["refined"] >= 1 and np.isfinite(models[0]["h"]).all() and not flags[spoiled].any()
    # the rows in their place carry nothing: the same model as over the set without them, at the same partials
    n, sums = F.refine_sums(bad, start[0]["h"], 3.0)
    zeroed = np.where(keep[:, None], rows, np.float32(0))      # rows at (0, 0, 0, 0) are far from the model: no inliers either
    n0, sums0 = F.refine_sums(zeroed, start[0]["h"], 3.0)
    assert n == n0 > 100 and R.same_bits(sums, sums0)


def test_equal_query_points():
    """All query points equal: the spread d is 0, the round fails at the normalisation."""
    rng = np.random.default_rng(12)
    rows = np.concatenate([np.full((50, 2), 40.0), 45.0 + rng.random((50, 2))], axis=1).astype(np.float32)
    start = F.model_of([[1, 0, 5.5], [0, 1, 5.5], [0, 0, 1]])
    n, _ = F.refine_sums(rows, start[0]["h"], 3.0)
    assert n == -1 - 50
    models, flags = F.refine(rows, start, None, 3.0, 8)
    assert models[0]["refined"] == 0 and models[0]["inliers"] == 50 == flags.sum() and R.same_bits(models[0]["h"], start[0]["h"])
