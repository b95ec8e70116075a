"""The host checker of 8-bit descriptor matching (tests/match_u8_ref.py: hostmath_quantize, hostmath_match_knn2_u8) against
numpy restatements that share no code with it.  No GPU.  Every comparison is exact."""
import numpy as np
import pytest

import match_ref as M
import match_u8_ref as U


def test_quantiser_kats():
    assert (U.quantize_flat(U.KAT_IN) == U.KAT_OUT).all()
    assert (U.quantize_np(U.KAT_IN) == U.KAT_OUT).all()


def test_quantiser_rounding_edges():
    """For every k the float nearest to (k + 0.5) / 255 and its two neighbours: fmaf's single rounding decides on which side of
    k + 1 the sum falls."""
    k = np.arange(255, dtype=np.float64)
    mid = ((k + 0.5) / 255.0).astype(np.float32)
    v = np.concatenate([np.nextafter(mid, np.float32(-1)), mid, np.nextafter(mid, np.float32(2))])
    got = U.quantize_flat(v)
    assert (got == U.quantize_np(v)).all()
    # each of the three is k or k + 1, in ascending order; which one is the rounding's business (near 255 a step of v is less
    # than half a step of t), and both answers occur
    steps = got.reshape(3, 255).astype(int) - np.arange(255)
    assert set(np.unique(steps)) == {0, 1} and (np.diff(steps, axis=0) >= 0).all()
    assert (steps[2] == 1).all()     # above the edge the exact sum is >= k + 1, which is a float: no rounding goes below it


def test_quantiser_random():
    rng = np.random.default_rng(0)
    v = (rng.random(100000) * 1.2 - 0.1).astype(np.float32)
    got = U.quantize_flat(v)
    assert (got == U.quantize_np(v)).all()
    assert got.min() == 0 and got.max() == 255
    inside = (v >= 0) & (v <= 1)
    assert np.abs(got[inside].astype(np.float64) - v[inside].astype(np.float64) * 255).max() <= 0.5 + 1e-4


def _same(got, want):
    assert M.same_bits(got[0], want[0]), np.nonzero((got[0] != want[0]).any(axis=1))[0][:8]
    assert M.same_bits(got[1], want[1])


@pytest.mark.parametrize("gen", [U.desc_rows_u8, U.uniform_rows_u8], ids=["desc", "uniform"])
def test_checker_against_int64(gen):
    rng = np.random.default_rng(1)
    q, t = gen(rng, 300), gen(rng, 300)
    _same(U.knn2(q, t), U.knn2_np(q, t))
    qv, tv = (rng.random(300) < 0.7).astype(np.uint8), (rng.random(300) < 0.7).astype(np.uint8)
    got = U.knn2(q, t, qv, tv)
    _same(got, U.knn2_np(q, t, qv, tv))
    assert (got[0][qv == 0] == -1).all() and np.isposinf(got[1][qv == 0]).all()
    assert not np.isin(got[0], np.nonzero(tv == 0)[0]).any()
    _same(U.knn2(q, t, None, tv), U.knn2_np(q, t, None, tv))
    # the empty sides and a single train row
    for nq, nt in ((0, 5), (5, 0), (3, 1)):
        got = U.knn2(q[:nq], t[:nt])
        _same(got, U.knn2_np(q[:nq], t[:nt]))
        assert got[0].shape == (nq, 2) and (got[0][:, 1] == -1).all()


def test_checker_duplicates():
    rng = np.random.default_rng(2)
    t = U.desc_rows_u8(rng, 300)
    t[200] = t[17]
    t[299] = t[100]
    idx, dist = U.knn2(t[[17, 100, 200]], t)
    assert idx.tolist() == [[17, 200], [100, 299], [17, 200]] and (dist == 0).all()
    _same((idx, dist), U.knn2_np(t[[17, 100, 200]], t))


def test_checker_extremes():
    """All 0, all 255, all 127, all 128, alternating 0 / 255 against each other: the largest distance, 128 * 255^2 = 8 323 200, is
    a float; a sign or overflow error of the a - 128 form shows here."""
    e = U.EXTREMES
    d = U.dist_matrix(e, e)
    assert d.max() == 8323200 and d[0, 1] == 8323200 and d[2, 3] == 128 and d[0, 4] == 64 * 255 * 255
    assert np.float32(8323200) == 8323200
    for i in range(5):
        others = np.delete(np.arange(5), i)
        got = U.knn2(e[i:i + 1], e[others])
        _same(got, U.knn2_np(e[i:i + 1], e[others]))
        assert got[1][0, 0] == d[i, others].min()
    idx, dist = U.knn2(e[:1], e[1:2])
    assert idx.tolist() == [[0, -1]] and dist[0, 0] == 8323200 and np.isposinf(dist[0, 1])


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 0.7, 0.8, 1.0])
def test_filter_over_checker(ratio, cross):
    """The numpy filter of the float matcher applies unchanged to the integer top-2: the same float32 ratio arithmetic over
    distances that happen to be integers; checked here against a plain loop."""
    rng = np.random.default_rng(3)
    q, t = U.desc_rows_u8(rng, 150), U.desc_rows_u8(rng, 140)
    t[7] = q[3]
    t[8] = q[3]           # a tie at distance 0: 0 < r2 * 0 is false, the ratio test drops it
    fwd, rev = U.knn2(q, t), U.knn2(t, q)
    got = M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0])
    want = []
    r2 = np.float32(ratio) * np.float32(ratio)
    for i in range(q.shape[0]):
        j = int(fwd[0][i, 0])
        if j < 0:
            continue
        if ratio != 0 and not (fwd[1][i, 0] < np.float32(r2 * fwd[1][i, 1])):
            continue
        if cross and rev[0][j, 0] != i:
            continue
        want.append((i, j, fwd[1][i, 0], fwd[1][i, 1]))
    assert [tuple(r) for r in got.tolist()] == [(a, b, float(c), float(d)) for a, b, c, d in want]
    assert (3 in got["query"].tolist()) == (ratio == 0)
