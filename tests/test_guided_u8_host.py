"""Guided matching on 8-bit descriptors, the host side (no GPU): the predicates' split parts (hostmath_guided_admissible_split,
composed as the tile kernel composes them) and the plain-loop checker hostmath_match_knn2_guided_u8, against numpy restatements
that share no code with the library (guided_ref.admissible, match_u8_ref.dist_matrix, guided_ref.top2)."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as G
import match_u8_ref as U

KINDS = ["homography", "fundamental"]


def _p(a, dtype):
    assert a is None or (a.dtype == dtype and a.flags.c_contiguous)      # the address of the array itself, not of a temporary
    return None if a is None else C.c_void_p(a.ctypes.data)


def split_admissible(kind, model, q_xy, t_xy, threshold, reverse):
    q_xy, t_xy = np.ascontiguousarray(q_xy, np.float32), np.ascontiguousarray(t_xy, np.float32)
    out = np.full((q_xy.shape[0], t_xy.shape[0]), 7, np.uint8)
    U.hostmath().hostmath_guided_admissible_split(G.KINDS[kind], _p(model, np.float32), C.c_float(threshold), _p(q_xy, np.float32),
                                                  C.c_longlong(q_xy.shape[0]), _p(t_xy, np.float32), C.c_longlong(t_xy.shape[0]),
                                                  int(reverse), _p(out, np.uint8))
    return out


def knn2_u8_numpy(q, t, q_xy, t_xy, kind, model, threshold, q_valid=None, t_valid=None, reverse=False):
    """The definition in numpy; tests/test_guided_u8_gpu.py holds the GPU to it."""
    d = U.dist_matrix(q, t).astype(np.float32)
    qv = np.ones(d.shape[0], bool) if q_valid is None else np.asarray(q_valid) != 0
    tv = np.ones(d.shape[1], bool) if t_valid is None else np.asarray(t_valid) != 0
    cand = G.admissible(kind, model, q_xy, t_xy, threshold) & qv[:, None] & tv[None]
    return G.top2(d.T, cand.T) if reverse else G.top2(d, cand)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_split_parts_compose_the_predicate(kind, reverse):
    rng = np.random.default_rng(12)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 129, 257, kind)
    bad = np.array([[np.nan, 5], [5, np.nan], [np.inf, 5], [5, -np.inf], [-0.0, 7], [7, -0.0], [-0.0, -0.0]], np.float32)
    q_xy[3:10], t_xy[40:47] = bad, bad
    every, zero = G.IDENTITY if kind == "homography" else G.F_ADMIT_ALL, np.zeros(9, np.float32)
    seen = 0
    for m, threshold in ((model, thr), (model, thr / 16), (model, 1e30), (every, 1e30), (zero, thr), (zero, 1e30), (-model, thr)):
        want = G.admissible(kind, m, q_xy, t_xy, threshold)
        got = split_admissible(kind, m, q_xy, t_xy, threshold, reverse)
        assert (got == want).all(), (threshold, np.argwhere(got != want)[:4])
        assert m.any() or not got.any()
        seen += int(want.sum())
    assert seen > 10000
    assert not split_admissible(kind, every, q_xy, t_xy, 1e30, reverse)[3:7].any()      # NaN and inf rows admit nothing


@pytest.mark.parametrize("kind", KINDS)
def test_checker_against_numpy(kind):
    rng = np.random.default_rng(13)
    q, t = U.desc_rows_u8(rng, 129), U.desc_rows_u8(rng, 257)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 129, 257, kind)
    t[100], t_xy[100] = t[7], t_xy[7]               # a tie: the lower index first
    qv, tv = (rng.random(129) < 0.8).astype(np.uint8), (rng.random(257) < 0.8).astype(np.uint8)
    for a, b in ((None, None), (qv, tv)):
        for reverse in (False, True):
            n = 257 if reverse else 129
            idx, dist = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
            U.hostmath().hostmath_match_knn2_guided_u8(_p(q, np.uint8), _p(a, np.uint8), _p(q_xy, np.float32), C.c_longlong(129), _p(t, np.uint8),
                                                       _p(b, np.uint8), _p(t_xy, np.float32), C.c_longlong(257), G.KINDS[kind],
                                                       _p(model, np.float32), C.c_float(thr), int(reverse), _p(idx, np.int32), _p(dist, np.float32))
            want = knn2_u8_numpy(q, t, q_xy, t_xy, kind, model, thr, a, b, reverse)
            assert G.same_bits(idx, want[0]) and G.same_bits(dist, want[1]) and (idx[:, 1] >= 0).sum() > 50
