"""The host checker of descriptor matching (hostmath_match_knn2) against numpy float64, and the rules of the definition
(include/sift_hip.h, "descriptor matching") on hand-built rows.  No GPU: the GPU matcher is then held to this checker bit for
bit (tests/test_match_gpu.py).

The error bound.  u = 2^-24, g(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).
d2 = fl(fl(na + nb) - 2 dot) with na, nb, dot fmaf chains of 128 steps over exactly representable inputs:
  * na and nb each pass 128 chain roundings, the add and the subtract: 130 roundings, every term a[k]^2 >= 0, so their
    share of the error is at most g(130) (n(a) + n(b));
  * 2 dot passes 128 chain roundings and the subtract (the doubling is exact): at most g(129) * 2 sum|a[k] b[k]|
    <= g(129) (n(a) + n(b)), since 2 |x y| <= x^2 + y^2;
  * the clamp at 0 moves the value towards the true one, which is >= 0.
So |d2 - d2_64| <= 2 g(130) (n64(a) + n64(b)); the float64 reference's own error is 2^-29 of that."""
import numpy as np
import pytest

import match_ref as M

U = 2.0 ** -24
G = 130 * U / (1 - 130 * U)


def _d64(q, t):
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    nq, nt = (q64 * q64).sum(axis=1), (t64 * t64).sum(axis=1)
    d = nq[:, None] + nt[None, :] - 2.0 * (q64 @ t64.T)
    return np.maximum(d, 0.0), 2 * G * (nq[:, None] + nt[None, :])


def _check_against_float64(q, t):
    idx, dist = M.knn2(q, t)
    d, bound = _d64(q, t)
    rows = np.arange(q.shape[0])
    worst = 0.0
    for k in range(min(2, t.shape[0])):
        err = np.abs(dist[:, k].astype(np.float64) - d[rows, idx[:, k]])
        worst = max(worst, float(err.max(initial=0.0)))
        assert (err <= bound[rows, idx[:, k]]).all(), (k, float(err.max()))
    # indices: wherever float64 separates the competitors by more than twice the bound
    order = np.argsort(d, axis=1, kind="stable")
    ds = np.take_along_axis(d, order, axis=1)
    bmax = bound.max(axis=1)
    clear0 = ds[:, 1] - ds[:, 0] > 2 * bmax if t.shape[0] > 1 else np.ones(q.shape[0], bool)
    assert (idx[clear0, 0] == order[clear0, 0]).all()
    if t.shape[0] > 2:
        clear1 = clear0 & (ds[:, 2] - ds[:, 1] > 2 * bmax)
        assert (idx[clear1, 1] == order[clear1, 1]).all()
        assert clear1.sum() > 0
    return worst, int(clear0.sum())


def test_checker_against_float64_generated_rows():
    rng = np.random.default_rng(5)
    for gen in (M.desc_rows, M.uniform_rows):
        worst, clear = _check_against_float64(gen(rng, 150), gen(rng, 170))
        assert clear > 100
        print(gen.__name__, "largest |d2 - d2_64|:", worst)


def test_checker_against_float64_real_descriptors():
    """The descriptors of two views of one frame, 8 columns apart (the oracle's: no GPU here)."""
    import oracle_lib as O
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    sets = []
    for x0 in (0, 8):
        kp, desc = O.OracleRun(np.ascontiguousarray(big[:, x0:x0 + 256]), 3, 3).points("final")
        sets.append(np.ascontiguousarray(desc, np.float32))
    assert sets[0].shape[0] > 100 and sets[1].shape[0] > 100
    worst, clear = _check_against_float64(sets[0], sets[1])
    print("rows:", sets[0].shape[0], sets[1].shape[0], "largest |d2 - d2_64|:", worst, "rows with a clear best:", clear)
    # symmetric bit for bit, and a row is at distance 0 from itself
    idx, dist = M.knn2(sets[0], sets[0])
    assert (dist[:, 0] == 0).all()


def test_checker_rules_on_hand_built_rows():
    e = np.eye(128, dtype=np.float32)
    t = np.stack([e[0] * 3, e[1] * 4, e[0] * 3, e[2]])          # rows 0 and 2 are the same
    q = np.stack([e[0] * 3, e[1] * 4, e[5]])
    idx, dist = M.knn2(q, t)
    assert idx[0].tolist() == [0, 2] and dist[0].tolist() == [0.0, 0.0]      # the lower index wins, the second is the other copy
    assert idx[1].tolist() == [1, 3] and dist[1].tolist() == [0.0, 17.0]
    assert idx[2].tolist() == [3, 0] and dist[2].tolist() == [2.0, 10.0]     # 10 = 1 + 9 for rows 0 and 2: row 0 first
    # masks: an invalid train row never appears, an invalid query row has no entry
    idx, dist = M.knn2(q, t, q_valid=[1, 0, 1], t_valid=[0, 1, 1, 1])
    assert idx[0].tolist() == [2, 3] and dist[0].tolist() == [0.0, 10.0]
    assert idx[1].tolist() == [-1, -1] and np.isinf(dist[1]).all()
    # one train row: no second; none: nothing
    idx, dist = M.knn2(q, t[1:2])
    assert idx[:, 0].tolist() == [0, 0, 0] and idx[:, 1].tolist() == [-1, -1, -1] and np.isinf(dist[:, 1]).all()
    idx, dist = M.knn2(q, t[:0])
    assert (idx == -1).all() and np.isinf(dist).all() and (dist > 0).all()
    idx, dist = M.knn2(q[:0], t)
    assert idx.shape == (0, 2)
    # a NaN distance is no candidate; +inf in a row makes its distances NaN (inf - inf) or +inf, and +inf is a candidate
    tn = t.copy()
    tn[0, 7] = np.nan
    idx, dist = M.knn2(q, tn)
    assert idx[0].tolist() == [2, 3] and 0 not in idx.ravel().tolist()
    ti = t.copy()
    ti[1, 1] = np.inf
    idx, dist = M.knn2(q[2:3], ti[1:2])          # n(b) = inf, dot = 0 * inf -> NaN: no candidate
    assert idx[0].tolist() == [-1, -1]
    # symmetry, bit for bit
    rng = np.random.default_rng(1)
    a, b = M.uniform_rows(rng, 40), M.uniform_rows(rng, 1)
    _, dab = M.knn2(a, b)
    for i in range(40):
        _, dba = M.knn2(b, a[i:i + 1])
        assert dba[0, 0].tobytes() == dab[i, 0].tobytes()


def test_entry_points_fail_without_a_context():
    """No CPU path: without a context (there is none without a GPU) the three calls return an error and its text."""
    import ctypes as C
    from sift_amd import _lib
    L = _lib.load()
    err = C.create_string_buffer(256)
    off = np.zeros(2, np.int64)
    p = np.zeros(1, np.int32)
    prm = _lib.MatchParams(0.8, 0)
    assert L.sift_hip_knn2(None, None, None, 1, off, 1, p, p, None, None, err, 256) == _lib.EINVAL and err.value
    assert L.sift_hip_match(None, None, None, 1, off, 1, p, p, C.byref(prm), None, p, None, err, 256) == _lib.EINVAL
    assert L.sift_hip_result_match(None, 1, p, p, C.byref(prm), None, p, None, err, 256) == _lib.EINVAL
