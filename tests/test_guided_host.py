"""The host checker of guided matching (hostmath_match_knn2_guided) against a numpy restatement of the definition
(include/sift_hip.h, "guided matching"; tests/guided_ref.py: the fmaf chain and the two predicates in float32, a stable
(d2, j) order), and the property that motivates the feature.  No GPU: the GPU matcher is then held to this checker bit for bit
(tests/test_guided_gpu.py)."""
import numpy as np
import pytest

import guided_ref as G
import match_ref as M

KINDS = ["homography", "fundamental"]
ZERO = np.zeros(9, np.float32)


def _rows(kind, seed=21, nq=130, nt=150):
    """130 x 150 rows with duplicate descriptors, tied distances, NaN / inf coordinates and invalid rows."""
    rng = np.random.default_rng(seed)
    q, t = M.desc_rows(rng, nq), M.desc_rows(rng, nt)
    q_xy, t_xy, model, thr = G.banded_scene(rng, nq, nt, kind)
    t[40] = t[3]                      # duplicates: equal distances to every query row
    t[149] = t[3]
    q[7] = t[3]                       # and a query row at distance 0 from all three
    line = model.astype(np.float64).reshape(3, 3) @ [q_xy[7, 0], q_xy[7, 1], 1.0]
    # row 3 where query row 7 admits it: at its transferred point / on its epipolar line
    t_xy[3] = line[:2] / line[2] if kind == "homography" else [1000.0, -(line[0] * 1000.0 + line[2]) / line[1]]
    t_xy[40] = t_xy[3]                # the two copies at one place: both admissible or neither
    q[8] = q[9]                       # two query rows tie for every train row (the reverse best)
    q_xy[8] = q_xy[9]
    t_xy[11, 0] = np.nan
    t_xy[12, 1] = np.inf
    q_xy[13, 1] = np.nan
    q_xy[14, 0] = -np.inf
    qv, tv = rng.random(nq) < 0.85, rng.random(nt) < 0.85
    qv[[7, 8, 9, 13, 14]] = True
    tv[[3, 40, 11, 12]] = True
    return q, t, q_xy, t_xy, model, thr, qv.astype(np.uint8), tv.astype(np.uint8)


def _same(got, want):
    assert G.same_bits(got[0], want[0]), np.nonzero((got[0] != want[0]).any(axis=1))[0][:8]
    assert G.same_bits(got[1], want[1])


def test_fma32_is_fmaf():
    """The restatement's fmaf against cases where rounding the double sum to float would round twice, and against exact
    integers."""
    one, eps = np.float32(1), np.float32(2.0 ** -24)
    # 1 + 2^-24 + 2^-53-ish: the double sum ties to even at 1 + 2^-24 exactly, the float rounding of which would go down
    a = np.float32(1 + 2.0 ** -12)
    got = G.fma32(np.array([a]), np.array([a]), np.array([np.float32(2.0 ** -30)]))[0]
    import math
    want = np.float32(math.fma(float(a), float(a), 2.0 ** -30)) if hasattr(math, "fma") else got
    assert got == want
    assert G.fma32(np.array([one]), np.array([eps]), np.array([one]))[0] == one          # a tie: to even
    x = np.arange(-50, 50, dtype=np.float32)
    assert (G.fma32(x, x, x) == x * x + x).all()


@pytest.mark.parametrize("kind", KINDS)
def test_checker_against_numpy(kind):
    q, t, q_xy, t_xy, model, thr, qv, tv = _rows(kind)
    adm = G.admissible(kind, model, q_xy, t_xy, thr)
    share = adm[np.isfinite(q_xy).all(axis=1)][:, np.isfinite(t_xy).all(axis=1)].mean()
    print(f"{kind}: the band admits {share:.3f} of the rows")
    assert 0.03 < share < 0.3
    assert not adm[:, [11, 12]].any() and not adm[[13, 14]].any()       # a NaN / inf coordinate: admissible for nothing, by nothing
    for masks in ((None, None), (qv, tv), (None, tv)):
        got = G.knn2(q, t, q_xy, t_xy, kind, model, thr, *masks)
        _same(got, G.knn2_numpy(q, t, q_xy, t_xy, kind, model, thr, *masks))
    assert got[0][13].tolist() == [-1, -1] and got[0][14].tolist() == [-1, -1]
    assert not np.isin(got[0], [11, 12]).any()
    # the duplicates: where row 3 is the best, its copy 40 at the same place is the second, at the same distance
    hit = got[0][:, 0] == 3
    assert hit.any() and (got[0][hit, 1] == 40).all() and (got[1][hit, 0] == got[1][hit, 1]).all()
    assert (got[0] != -1).any(axis=1).sum() > 60 and (got[0][:, 1] == -1).any()


@pytest.mark.parametrize("kind", KINDS)
def test_cross_check_reverse_best(kind):
    q, t, q_xy, t_xy, model, thr, qv, tv = _rows(kind)
    for masks in ((None, None), (qv, tv)):
        got = G.knn2(q, t, q_xy, t_xy, kind, model, thr, *masks, reverse=True)
        assert got[0].shape == (150, 2)
        _same(got, G.knn2_numpy(q, t, q_xy, t_xy, kind, model, thr, *masks, reverse=True))
    # rows 8 and 9 of the query set are one row at one place: wherever 8 is the reverse best, 9 is the second at its distance
    got = G.knn2(q, t, q_xy, t_xy, kind, model, thr, reverse=True)
    hit = got[0][:, 0] == 8
    assert (got[0][hit, 1] == 9).all() and (got[1][hit, 0] == got[1][hit, 1]).all() and 9 not in got[0][:, 0].tolist()
    # the same model in the same direction: the reverse list holds (j, i) exactly when i admits j
    adm = G.admissible(kind, model, q_xy, t_xy, thr)
    j = np.nonzero(got[0][:, 0] >= 0)[0]
    assert adm[got[0][j, 0], j].all()


@pytest.mark.parametrize("kind", KINDS)
def test_admit_all_and_admit_nothing(kind):
    q, t, q_xy, t_xy, _, _, qv, tv = _rows(kind)
    finite_q, finite_t = np.isfinite(q_xy).all(axis=1), np.isfinite(t_xy).all(axis=1)
    q_xy, t_xy = np.where(finite_q[:, None], q_xy, 5), np.where(finite_t[:, None], t_xy, 5)
    model = G.IDENTITY if kind == "homography" else G.F_ADMIT_ALL
    assert G.admissible(kind, model, q_xy, t_xy, 1e30).all()
    for masks in ((None, None), (qv, tv)):
        _same(G.knn2(q, t, q_xy, t_xy, kind, model, 1e30, *masks), M.knn2(q, t, *masks))
        _same(G.knn2(q, t, q_xy, t_xy, kind, model, 1e30, *masks, reverse=True), M.knn2(t, q, *masks[::-1]))
        idx, dist = G.knn2(q, t, q_xy, t_xy, kind, ZERO, 1e30, *masks)
        assert (idx == -1).all() and np.isposinf(dist).all()
        idx, dist = G.knn2(q, t, q_xy, t_xy, kind, ZERO, 3.0, *masks, reverse=True)
        assert (idx == -1).all() and np.isposinf(dist).all()


def _unguided_float64(q, t, ratio):
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    d = (q64 * q64).sum(axis=1)[:, None] + (t64 * t64).sum(axis=1)[None] - 2.0 * q64 @ t64.T
    order = np.argsort(d, axis=1, kind="stable")
    best = np.take_along_axis(d, order[:, :2], axis=1)
    return order[:, 0], best[:, 0] < ratio * ratio * best[:, 1]


def _guided_float64(kind, q, t, q_xy, t_xy, model, thr, ratio):
    """The judge of the twin scenes: float64 distances, the band in float64 pixels (reprojection error / Sampson distance)."""
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    d = (q64 * q64).sum(axis=1)[:, None] + (t64 * t64).sum(axis=1)[None] - 2.0 * q64 @ t64.T
    m = model.astype(np.float64).reshape(3, 3)
    qh = np.concatenate([q_xy.astype(np.float64), np.ones((len(q_xy), 1))], axis=1)
    th = np.concatenate([t_xy.astype(np.float64), np.ones((len(t_xy), 1))], axis=1)
    if kind == "homography":
        p = qh @ m.T
        e2 = ((p[:, None, :2] / p[:, None, 2:] - th[None, :, :2]) ** 2).sum(axis=2)
    else:
        fq, ftt = qh @ m.T, th @ m                     # F q per query row, F^T t per train row
        r = fq @ th.T
        e2 = r * r / ((fq[:, :2] ** 2).sum(axis=1)[:, None] + (ftt[:, :2] ** 2).sum(axis=1)[None])
    d = np.where(e2 <= thr * thr, d, np.inf)
    order = np.argsort(d, axis=1, kind="stable")
    best = np.take_along_axis(d, order[:, :2], axis=1)
    return order[:, 0], np.isfinite(best[:, 0]) & (best[:, 0] < ratio * ratio * best[:, 1])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", KINDS)
def test_twins_are_lost_unguided_and_found_guided(kind, seed):
    """400 true pairs, rows 0 .. 199 with a twin descriptor 50 to 300 px off the target; ratio 0.8, band 3 px.  The unguided
    ratio test drops nearly every twinned row; guided matching returns exactly the 400 true pairs.  The float64 numpy
    restatement is the judge of the generator, the host loop is the code under test."""
    q, t, q_xy, t_xy, model, truth, twin_of = G.twin_scene(seed, kind)
    assert q.shape == (400, 128) and t.shape == (600, 128) and twin_of.shape == (200,)
    # the judge
    best64, keep64 = _unguided_float64(q, t, 0.8)
    g64, gkeep64 = _guided_float64(kind, q, t, q_xy, t_xy, model, 3.0, 0.8)
    print(f"{kind} seed {seed}: float64 unguided keeps {int(keep64.sum())} rows, {int(keep64[:200].sum())} of the twinned; "
          f"guided keeps {int(gkeep64.sum())}")
    assert gkeep64.all() and (g64 == truth).all()
    assert keep64[:200].sum() <= 10 and keep64[200:].all()
    # unguided: hostmath_match_knn2 plus the ratio test
    idx, dist = M.knn2(q, t)
    keep = G.ratio_keep(idx, dist, 0.8)
    print(f"    checker: unguided keeps {int(keep.sum())} rows, {int(keep[:200].sum())} of the 200 twinned")
    assert keep[:200].sum() <= 10
    assert np.isin(idx[:200, 0], np.concatenate([truth[:200], twin_of])).all()
    # guided: every row, its true partner
    rec = G.matches(q, t, q_xy, t_xy, kind, model, 3.0, 0.8, False)
    assert rec.size == 400 and (rec["query"] == np.arange(400)).all() and (rec["train"] == truth).all()


def test_entry_points_fail_without_a_context():
    """No CPU path: without a context the three guided calls return an error and its text."""
    import ctypes as C
    from sift_amd import _lib
    L = _lib.load()
    err = C.create_string_buffer(256)
    off = np.zeros(2, np.int64)
    p = np.zeros(1, np.int32)
    prm = _lib.MatchParams(0.8, 0)
    gp = _lib.GuideParams(0, 3.0)
    assert L.sift_hip_knn2_guided(None, None, None, None, 1, off, 1, p, p, C.byref(gp), None, None, None, err, 256) == _lib.EINVAL and err.value
    assert L.sift_hip_match_guided(None, None, None, None, 1, off, 1, p, p, C.byref(prm), C.byref(gp), None, None, p, None, err, 256) == _lib.EINVAL
    assert L.sift_hip_result_match_guided(None, 1, p, p, C.byref(prm), C.byref(gp), None, None, p, None, err, 256) == _lib.EINVAL
    assert C.sizeof(_lib.GuideParams) == 8
