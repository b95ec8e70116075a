"""The warp's definition (sift_amd/csrc/warp_math.h) through its host loop: exact cases against numpy indexing, general models
against a float64 restatement within the float error of the map."""
import numpy as np
import pytest

import warp_ref as WR


def _img(w, h, seed=0):
    return (np.random.default_rng(seed + 7 * w + h).random((h, w)) * 255).astype(np.float32)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (65, 17)])
def test_exact_cases(w, h, interp):
    img, fill = _img(w, h), np.float32(-7.5)
    out, mask = WR.host(img[None], [WR.translation(0, 0)], fill=fill, interp=interp)
    assert out[0].tobytes() == img.tobytes() and mask.all()
    # an integer translation on a canvas that exceeds the frame: output (x, y) is the source at (x + ox + dx, y + oy + dy)
    (dx, dy), (ox, oy), (oh, ow) = (2, -1), (-3, 1), (h + 4, w + 5)
    out, mask = WR.host(img[None], [WR.translation(dx, dy)], None, (oh, ow), (ox, oy), fill, interp)
    ys, xs = np.mgrid[0:oh, 0:ow]
    sx, sy = xs + ox + dx, ys + oy + dy
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    want = np.where(inside, img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], fill)
    assert out[0].tobytes() == want.tobytes() and (mask[0] == inside).all()
    out, mask = WR.host(img[None], [WR.rot90(w)], None, (w, h), (0, 0), fill, interp)
    assert out[0].tobytes() == np.ascontiguousarray(np.rot90(img)).tobytes() and mask.all()
    for model in ([0.0] * 9, [1, 0, 0, 0, float("nan"), 0, 0, 0, 1]):
        out, mask = WR.host(img[None], [model], fill=fill, interp=interp)
        assert (out == fill).all() and not mask.any()


SRC, OUT = (97, 61), (80, 48)   # (w, h)
GENERAL = {
    "rot30": WR.rotation(30.0, 0.75, SRC, OUT),
    "projective": WR.projective(WR.rotation(10.0, 0.9, SRC, OUT), -0.004, -0.003),          # W >= 0.54 on the canvas
    "sign_change": WR.projective(WR.rotation(10.0, 0.9, SRC, OUT), -1.0 / 100, -1.0 / 80),   # W = 0 on a line through the canvas
}


@pytest.mark.parametrize("name", list(GENERAL))
def test_host_loop_against_float64(name):
    """tol per pixel from the two fmaf roundings of X, Y and W: du = 2^-22 (Sx + |u| Sw) / |W|, dv likewise (the factor 2 over
    2^-23 covers the quotient's rounding and second-order terms); the value moves by at most G (du + dv), G the largest difference
    between neighbouring source pixels, plus 2^-21 max|img| for the three fmaf of the interpolation and its two differences."""
    img = _img(*SRC, seed=3)
    model = np.array(GENERAL[name], np.float32)
    out, mask = WR.host(img[None], [model], None, OUT[::-1])
    r = WR.restate(img, model, OUT[::-1])
    with np.errstate(all="ignore"):
        du = 2.0 ** -22 * (r["Sx"] + abs(r["u"]) * r["Sw"]) / abs(r["W"])
        dv = 2.0 ** -22 * (r["Sy"] + abs(r["v"]) * r["Sw"]) / abs(r["W"])
        near = (abs(r["W"]) < 2.0 ** -10) | ~np.isfinite(du + dv)
        for c, d, hi in ((r["u"], du, SRC[0] - 1), (r["v"], dv, SRC[1] - 1)):
            near |= (abs(c) <= d) | (abs(c - hi) <= d)
    assert near.mean() <= 0.01, near.mean()
    keep = ~near
    assert (mask[0][keep] == r["covered"][keep]).all()
    assert r["covered"].mean() > 0.1 and (name != "sign_change" or (r["W"] < 0).mean() > 0.05)   # the case is what its name says
    G = max(abs(np.diff(img.astype(np.float64), axis=0)).max(), abs(np.diff(img.astype(np.float64), axis=1)).max())
    tol = G * (du + dv) + 2.0 ** -21 * float(abs(img).max())
    sel = keep & r["covered"]
    err = abs(out[0].astype(np.float64) - r["value"])
    print(name, "left out", int(near.sum()), "max err", err[sel].max(), "min slack", (tol - err)[sel].min())
    assert (err[sel] <= tol[sel]).all()
    assert (out[0][keep & ~r["covered"]] == 0.0).all()
