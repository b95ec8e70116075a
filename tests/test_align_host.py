"""align_math.h on the host (hostmath_align_homography) against the float64 Gauss-Newton of tests/align_ref.py: the fixed-order
sums, convergence on the analytic fixture, and the stopping cases."""
import functools
import math

import numpy as np
import pytest

import align_ref as A
from sift_amd import _lib

IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]


@functools.lru_cache(maxsize=None)
def _converged():
    return A.host(A.fixture(), [(0, 1)], A.records([A.H_START]), rounds=8)[1][0]


def test_sums_against_float64():
    """Relative to sqrt(G_ii G_jj), the scale Cauchy-Schwarz gives entry (i, j).  Measured on these three cases: 1.17e-5 at the
    worst (entry (8, 11) at the converged model, where the residual column is the rounding of its own subtraction); the bound is
    8 x that, DESIGN.md section 3m."""
    imgs, end = A.fixture(), _converged()
    worst = 0.0
    for model, gain, bias in ((A.H_START, 1.0, 0.0), (end["h"], float(end["gain"]), float(end["bias"])), ([1, 0, 0.5, 0, 1, 0.5, 0, 0, 1], 1.0, 0.0)):
        got = A.host_sums(imgs, model, gain, bias)
        G, n = A.gram64(imgs[0], imgs[1], np.float32(model), np.float32(gain), np.float32(bias))
        d = np.sqrt(np.diag(G))
        worst = max(worst, float((np.abs(got[:78] - G[A.I, A.J]) / (d[A.I] * d[A.J])).max()))
        assert got[78] == n > 40000 and got[79] == 0
    print("largest relative deviation of a sum:", worst)
    assert worst <= 8 * 1.18e-5


def test_convergence():
    """The float64 reference alone takes the start's 1.6 pixels to 0.00283; the host loop ends 1.4e-7 pixel from it (measured), the
    margin is that gap doubled.  The bilinear patch damps the fixture's sinusoids (periods from 20 pixels) by up to 1.2 %: the
    gain is 1.25 to within 0.02 and the bias -12.5 to within 0.02 x 128."""
    imgs, end = A.fixture(), _converged()
    ref = A.gauss_newton64(imgs[0], imgs[1], A.H_START, 8)
    ref_err, err = A.corner_error(ref[0], A.H_TRUE, A.W, A.H), A.corner_error(end["h"], A.H_TRUE, A.W, A.H)
    print("corner error: start", A.corner_error(A.H_START, A.H_TRUE, A.W, A.H), "float64", ref_err, "host", err)
    assert ref_err < 0.05 and abs(ref[1] - 1.25) < 0.02 and abs(ref[2] + 12.5) < 2.56
    assert err <= ref_err + 3e-7
    assert abs(end["gain"] - ref[1]) < 1e-5 and abs(end["bias"] - ref[2]) < 1e-3
    assert end["rms"] < 0.01 * end["rms0"] and end["rounds"] >= 4 and math.isclose(end["rms0"], ref[3], rel_tol=1e-5)


def _low_contrast():
    """A train frame of a tenth of the query's contrast, a fifth of a period off: the step wants a gain of ten and lands where
    the frames do not correlate, so E / n rises at the first step."""
    y, x = np.mgrid[0:64, 0:64].astype(np.float64)
    f = lambda x, y, amp: 128 + amp * np.sin(2 * math.pi * x / 8) * np.sin(2 * math.pi * y / 8)
    return np.stack([f(x, y, 50), f(x + 1.6, y + 1.6, 5)]).astype(np.float32)


@pytest.mark.parametrize("imgs,model,iteration,status,pixels", [
    (A.fixture, [0] * 9, -1, _lib.ALIGN_NO_MODEL, 0),
    (A.fixture, [0] * 9, 0, _lib.ALIGN_TOO_FEW, 0),                              # W = 0 everywhere: nothing is covered
    (A.fixture, [1, 0, 250, 0, 1, 0, 0, 0, 1], 0, _lib.ALIGN_TOO_FEW, 3 * 188),  # columns 2 .. 4 inside the border of 2
    (lambda: np.full((2, 64, 64), 5, np.float32), IDENTITY, 0, _lib.ALIGN_SINGULAR, 60 * 60),
    (_low_contrast, IDENTITY, 0, _lib.ALIGN_ROSE, 60 * 60)])
def test_stopping_cases(imgs, model, iteration, status, pixels):
    models, out, _ = A.host(imgs(), [(0, 1)], A.records([model], iteration), rounds=4, min_pixels=1000)
    start = np.float32(model)
    assert out["status"][0] == status and out["rounds"][0] == 0 and out["pixels"][0] == pixels
    assert out["h"][0].tobytes() == start.tobytes() == models["h"][0].tobytes() and out["gain"][0] == 1 and out["bias"][0] == 0
    assert out["rms"][0] == out["rms0"][0] and models["iteration"][0] == iteration
