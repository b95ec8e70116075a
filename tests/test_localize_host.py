"""sift_amd/csrc/localize_math.h without a GPU: the host loop against the Python restatement, and against records known exactly."""
import numpy as np
import pytest

import localize_ref as LR

F = np.float32


def _one(stack, p, max_moves=5):
    got = LR.host(stack, [p[0]], [p[1]], [p[2]], max_moves)
    assert LR.same(got, LR.restate(stack, [p[0]], [p[1]], [p[2]], max_moves))
    return got[0]


def test_host_loop_equals_restatement():
    rng = np.random.default_rng(5)
    stack = (rng.random((5, 10, 12)) * 64 + 96).astype(np.float32)
    xs, ys, idx = rng.integers(1, 11, 500), rng.integers(1, 9, 500), rng.integers(1, 4, 500)
    for max_moves in (0, 1, 5, 8):
        got = LR.host(stack, xs, ys, idx, max_moves)
        assert LR.same(got, LR.restate(stack, xs, ys, idx, max_moves))
    assert set(got["status"]) >= {LR.OK, LR.LEFT_RANGE} and got["moves"].max() > 1
    got = LR.host(stack, xs, ys, idx, 5, 3, 0.5)   # octave 3 of a subpixel batch
    assert LR.same(got, LR.restate(stack, xs, ys, idx, 5, 3, 0.5))


@pytest.mark.parametrize("L", [3, 5])
def test_exact_quadratic_offsets(L):
    c = (6, 4, L // 2)
    v = (0.25, -0.375, 0.125)
    r = _one(LR.quadratic_stack(L, 12, 10, c, v), c)
    assert (r["status"], r["moves"]) == (LR.OK, 0) and (r["dx"], r["dy"], r["ds"]) == tuple(map(F, v))
    assert (r["x"], r["y"], r["value"]) == (F(6.25), F(3.625), F(100.0)) and (r["mx"], r["my"], r["mi"]) == (0, 0, 0)
    r = _one(LR.quadratic_stack(L, 12, 10, c, (0.75, 0, 0)), c)
    assert (r["status"], r["moves"], r["mx"], r["my"], r["mi"]) == (LR.OK, 1, 1, 0, 0) and (r["dx"], r["x"]) == (F(-0.25), F(6.75))
    r = _one(LR.quadratic_stack(3, 12, 10, (6, 4, 1), (0, 0, 0.75)), (6, 4, 1))
    assert (r["status"], r["moves"], r["x"], r["ds"], r["value"]) == (LR.LEFT_RANGE, 0, F(6), F(0), F(100 - 0.5 * 0.75 ** 2))
    r = _one(LR.quadratic_stack(5, 12, 10, (6, 4, 2), (0, 0, 0.75)), (6, 4, 2))
    assert (r["status"], r["mi"], r["ds"]) == (LR.OK, 1, F(-0.25))


def test_every_other_status():
    assert _one(np.full((3, 10, 12), 7, np.float32), (5, 5, 1))["status"] == LR.SINGULAR
    stack = LR.quadratic_stack(3, 12, 10, (6, 4, 1), (0, 0, 0))
    stack[2, 5, 7] = np.nan
    assert _one(stack, (6, 4, 1))["status"] == LR.NOT_FINITE
    assert _one(LR.quadratic_stack(3, 12, 10, (10, 4, 1), (0.75, 0, 0)), (10, 4, 1))["status"] == LR.LEFT_RANGE   # x = w - 2
    far = LR.quadratic_stack(3, 12, 10, (4, 4, 1), (3, 0, 0))
    r = _one(far, (4, 4, 1), 1)
    assert (r["status"], r["moves"], r["mx"], r["x"]) == (LR.NOT_CONVERGED, 1, 0, F(4))
    r = _one(far, (4, 4, 1), 5)
    assert (r["status"], r["moves"], r["mx"], r["dx"], r["x"]) == (LR.OK, 3, 3, F(0), F(7))
