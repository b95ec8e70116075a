"""The two-band compositor's definition (sift_amd/csrc/twoband_math.h) through its host loop: exact cases against float64 numpy
rounded after every operation, bitwise; general models against the un-rounded float64 restatement within the float error carried
through the passes and the blend; and a cropped canvas against the crop of the larger one, bitwise."""
import numpy as np
import pytest

import composite_ref as CR
import twoband_ref as TR
import warp_ref as WR
from test_warp_host import GENERAL, OUT, SRC, _img

OFFSETS, GAINS = [0, 5, 5, 8], [1.25, 0.5, 0.75, 1.5, 1.0, 0.875, 2.0, 1.0]


def gauss(radius, sigma):
    k = np.exp(-0.5 * (np.arange(radius + 1) / sigma) ** 2)
    return (k / (k[0] + 2 * k[1:].sum())).astype(np.float32)


def crop_case():
    """The GPU tests' largest case and its two canvases: (imgs, models, src, taps, gains, kw of the 129 x 49 canvas, kw of the 40 x 20
    canvas, the slices of the latter in the former)."""
    imgs = (np.random.default_rng(130 + 31 * 70).random((2, 70, 130)) * 255).astype(np.float32)
    big, small = dict(out_shape=(49, 129), origin=(-2, 1)), dict(out_shape=(20, 40), origin=(35, 12))
    return imgs, WR.job_models(130, 70, 129, 49), np.arange(8, dtype=np.int32) % 2, gauss(3, 1.0), GAINS, big, small, (slice(11, 31), slice(37, 77))


@pytest.mark.parametrize("gains", [None, [0.5, 2.0, 1.5, 1.0, 0.75]])
@pytest.mark.parametrize("taps", [[0.5, 0.25], [1.0]])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (65, 17)])
def test_exact_cases(w, h, interp, taps, gains):
    """Integer images in 1 .. 255, integer translations and rot90, dyadic taps and gains: every t is a small multiple of 1/4, every
    weight an integer, every tap sum a multiple of 1/16, so each product-and-sum of a chain and of the blend is exact in float64
    (operands of at most 24 bits whose exponents span far less than 53 bits) before its one rounding to float32 - that IS fmaf.
    L = ls / ln lies in [1/2, 510], so H = t - L is a multiple of 2^-24 below 2^9 and the final add is exact in float64 too.  A
    quotient of two floats formed in float64 and rounded to float32 is the correctly rounded quotient (53 >= 2 * 24 + 2 bits).
    With the single tap 1.0, L = t and H = 0: the feather blend, bit for bit."""
    imgs = np.floor(np.stack([_img(w, h, seed) for seed in (0, 1, 2)]) * (254.0 / 255.0)) + 1.0
    fill, (ox, oy), (oh, ow) = np.float32(-7.5), (-3, -2), (max(w, h) + 4, max(w, h) + 5)
    models = [WR.translation(2, -1), [0.0] * 9, WR.rot90(w), [1, 0, 0, 0, float("nan"), 0, 0, 0, 1], WR.translation(-1, 2)]
    src = [0, 1, 2, 0, 1]
    out, count = TR.host(imgs, models, taps, [0, 5, 5], src, (oh, ow), (ox, oy), fill, interp, gains)
    value, cnt, _ = TR.twoband64(imgs[src], models, taps, (oh, ow), (ox, oy), gains, rnd=lambda a: a.astype(np.float32).astype(np.float64))
    want = np.where(cnt > 0, value, fill).astype(np.float32)
    assert imgs.min() >= 1 and imgs.max() <= 255 and cnt.max() >= min(w * h, 2)   # the jobs overlap
    assert out[0].tobytes() == want.tobytes() and (count[0] == cnt).all()
    assert (out[1] == fill).all() and not count[1].any()   # the empty group
    if len(taps) == 1 and gains is None:
        feather, feather_count = CR.host(imgs, models, [0, 5, 5], src, (oh, ow), (ox, oy), fill, interp, 2)
        assert out.tobytes() == feather.tobytes() and count.tobytes() == feather_count.tobytes()


def _window(a, radius, op):
    """`op` over the (2R + 1)^2 window of every canvas pixel; `a` lives on the canvas widened by R."""
    oh, ow = a.shape[0] - 2 * radius, a.shape[1] - 2 * radius
    return op.reduce([a[dy:dy + oh, dx:dx + ow] for dy in range(2 * radius + 1) for dx in range(2 * radius + 1)])


def test_host_loop_against_float64():
    """Three jobs (rot30, projective, sign_change) of one canvas, R = 2, Gaussian taps.  Per job and lattice point, as
    test_composite_host.py has it: du = 2^-22 (Sx + |u| Sw) / |W|, dv likewise, and the job's value moves by at most e_j = G (du_j +
    dv_j) + 2^-21 max|img|.  L_j is a convex combination of the job's values in the pixel's window (non-negative taps over their own
    sum), so it moves by at most the largest e_j in the window, plus (2 (2R + 1) + 2) 2^-24 max|img| for the roundings of the two
    chains and the quotient.  H_j = t_j - L_j moves by e_j + dL_j and one rounding.  The low band then goes through the feather
    bound of that test with dL_j in e_j's place: sum wgt_j dL_j / wsum, the weights' own movement (du_j + dv_j and two roundings)
    times range(img) / wsum, and (n + 3) 2^-24 max|img| for the ordered adds and the division; the high band is the one of the job
    with the largest weight, and the last add rounds a number below 2 max|img| once.
    Left out: pixels within R of a lattice point that is within du, dv of a coverage edge of any job (coverage itself may differ
    there, and with it ln) - that test leaves out 7 of 3840 pixels on these inputs, so at most 7 * 25 = 175 here, a share of 0.046 -
    and pixels whose two largest weights are closer than the weights' movement, where the high band may come from either job."""
    R, taps = 2, gauss(2, 1.0)
    imgs = np.stack([_img(*SRC, seed=3 + k) for k in range(3)])
    models = np.array(list(GENERAL.values()), np.float32)
    out, count = TR.host(imgs, models, taps, None, None, OUT[::-1], (0, 0), -1.0, 1)
    value, cnt, jobs = TR.twoband64(imgs, models, taps, OUT[::-1])
    big, G = float(abs(imgs).max()), max(abs(np.diff(imgs.astype(np.float64), axis=1)).max(), abs(np.diff(imgs.astype(np.float64), axis=2)).max())
    crop = lambda a: a[R:-R, R:-R]
    near, dL, dH, dw = np.zeros(OUT[::-1], bool), [], [], []
    with np.errstate(all="ignore"):
        for job in jobs:
            r = job["wide"]
            du = 2.0 ** -22 * (r["Sx"] + abs(r["u"]) * r["Sw"]) / abs(r["W"])
            dv = 2.0 ** -22 * (r["Sy"] + abs(r["v"]) * r["Sw"]) / abs(r["W"])
            edge = (abs(r["W"]) < 2.0 ** -10) | ~np.isfinite(du + dv)
            for c, dc, hi in ((r["u"], du, SRC[0] - 1), (r["v"], dv, SRC[1] - 1)):
                edge |= (abs(c) <= dc) | (abs(c - hi) <= dc)
            near |= _window(edge, R, np.logical_or)
            e = np.where(r["covered"], G * (du + dv) + 2.0 ** -21 * big, 0.0)
            dL.append(_window(e, R, np.maximum) + (2 * (2 * R + 1) + 2) * 2.0 ** -24 * big)
            dH.append(crop(e) + dL[-1] + 2.0 ** -24 * big)
            dw.append(np.where(job["covered"], crop(du + dv) + 2.0 ** -22 * job["wgt"], 0.0))
        wsum = sum(job["wgt"] for job in jobs)
        wgts = np.stack([job["wgt"] for job in jobs])   # 0 where not covered; a covered pixel's is >= 1
        top = wgts.argmax(axis=0)                       # the first of equal weights, as the definition has it
        two = np.sort(wgts, axis=0)[-2:]
        near |= (cnt >= 2) & (two[1] - two[0] <= 2 * np.stack(dw).max(axis=0))
        tol = sum(job["wgt"] * dL[k] for k, job in enumerate(jobs)) / wsum + float(imgs.max() - imgs.min()) * sum(dw) / wsum
        tol = tol + (cnt + 3) * 2.0 ** -24 * big + np.choose(top, dH) + 2.0 ** -23 * big
    assert near.mean() <= 0.10, near.mean()
    keep = ~near
    assert (count[0][keep] == cnt[keep]).all() and (cnt[keep] >= 2).mean() > 0.1   # the jobs overlap
    sel = keep & (cnt > 0)
    err = abs(out[0].astype(np.float64) - value)
    print("left out", int(near.sum()), "max err", err[sel].max(), "min slack", (tol - err)[sel].min())
    assert (err[sel] <= tol[sel]).all()
    assert (out[0][keep & (cnt == 0)] == -1.0).all()


def test_crop_invariance():
    """A lattice point's value depends on the inputs alone: the 40 x 20 canvas at (35, 12) is [11:31, 37:77] of the 129 x 49 canvas at (-2, 1)."""
    imgs, models, src, taps, gains, big, small, where = crop_case()
    out, count = TR.host(imgs, models, taps, OFFSETS, src, fill=-1.0, gains=gains, **big)
    sub, sub_count = TR.host(imgs, models, taps, OFFSETS, src, fill=-1.0, gains=gains, **small)
    assert sub.tobytes() == np.ascontiguousarray(out[(slice(None),) + where]).tobytes()
    assert sub_count.tobytes() == np.ascontiguousarray(count[(slice(None),) + where]).tobytes()
    assert sub_count[0].max() >= 3 and not sub_count[1].any()
