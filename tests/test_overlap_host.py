"""overlap_math.h in the host loop against numpy (tests/overlap_ref.py): the statistics as integers, the gains against a float64
solve, what the gains do to differently exposed frames, and the compositor's host loop with gains."""
import numpy as np
import pytest

import composite_ref as CR
import overlap_ref as OR

# the host loop's largest relative deviation from numpy.linalg.solve on the cases below, measured on the CPU, is 5.27e-8
# (0.44 * 2^-23: the output's rounding to float dominates); the bound is 8 x that, and never below one float ulp near 1
GAIN_RTOL = max(8 * 5.27e-8, 2.0 ** -23)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h,ow,oh", OR.SHAPES)
def test_host_equals_numpy(w, h, ow, oh, interp):
    imgs, models, src, (stats, gains, status) = OR.case(w, h, ow, oh, interp)
    assert not stats[1].any() and not status.any()
    for c in (0, 2):
        a, b = OR.OFFSETS[c], OR.OFFSETS[c + 1]
        want = OR.numpy_stats(imgs, models[a:b], src[a:b], (oh, ow), OR.ORIGIN, 1.0, interp)
        assert (stats[c] == want).all()
        dev = np.abs(gains[a:b] / OR.numpy_gains(want, b - a) - 1).max()
        print(f"gains: largest relative deviation {dev:.3g}")
        assert dev <= GAIN_RTOL


def test_gains_level_the_exposures():
    imgs, models, shape = OR.exposure_fixture()
    want = OR.numpy_stats(imgs, models, None, shape)
    flat, ref = OR.exposure_residual(want, np.ones(3)), OR.exposure_residual(want, OR.numpy_gains(want, 3))
    stats, gains, status = OR.host(imgs, models, None, None, shape)
    got = OR.exposure_residual(stats[0], gains.astype(np.float64))
    print(f"residual: gains 1 {flat:.4g}, numpy {ref:.4g}, host loop {got:.4g}")
    assert (stats[0] == want).all() and not status.any()
    assert ref < 0.5 * flat and got < 0.5 * flat


@pytest.mark.parametrize("blend", [0, 1, 2])
def test_composite_with_gains(blend):
    imgs, models, src, _ = OR.case(65, 17, 63, 33, 1)
    kw = dict(offsets=OR.OFFSETS, src=src, out_shape=(33, 63), origin=OR.ORIGIN, fill=-1.0, interp=1, blend=blend)
    plain = CR.host(imgs, models, **kw)
    ones = OR.host_composite(imgs, models, np.ones(8, np.float32), **kw)
    assert ones[0].tobytes() == plain[0].tobytes() and ones[1].tobytes() == plain[1].tobytes()
    # powers of two: gain * value is exact, so a job's gain is its image's scale; jobs of image 0 get 0.5, of image 1 get 2
    gains = np.array([0.5, 2.0] * 4, np.float32)
    got = OR.host_composite(imgs, models, gains, **kw)
    want = CR.host(imgs * gains[:2, None, None], models, **kw)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
