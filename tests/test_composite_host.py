"""The compositor's definition (sift_amd/csrc/composite_math.h) through its host loop: exact integer cases against plain numpy,
bitwise, and general models against the float64 blend of warp_ref.restate within the float error carried through the blend."""
import numpy as np
import pytest

import composite_ref as CR
import warp_ref as WR
from test_warp_host import GENERAL, OUT, SRC, _img


@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (65, 17)])
def test_exact_cases(w, h, interp, blend):
    """Integer images, integer translations and rot90: every u, v, weight, product and sum is an integer below 2^24, so the
    float chain is exact up to the one division, and float32(a / b) from float64 is that division (53 >= 2 * 24 + 2 bits)."""
    imgs = np.floor(np.stack([_img(w, h, seed) for seed in (0, 1, 2)]))
    fill, (ox, oy), (oh, ow) = np.float32(-7.5), (-3, -2), (max(w, h) + 4, max(w, h) + 5)
    models = [WR.translation(2, -1), [0.0] * 9, WR.rot90(w), [1, 0, 0, 0, float("nan"), 0, 0, 0, 1], WR.translation(-1, 2)]
    src = [0, 1, 2, 0, 1]
    out, count = CR.host(imgs, models, [0, 5, 5], src, (oh, ow), (ox, oy), fill, interp, blend)
    ys, xs = np.mgrid[0:oh, 0:ow]
    X, Y = xs + ox, ys + oy
    acc, wsum, cnt, first = (np.zeros((oh, ow), np.int64) for _ in range(4))
    for k, (sx, sy) in ((0, (X + 2, Y - 1)), (2, (w - 1 - Y, X)), (1, (X - 1, Y + 2))):   # the three jobs that can cover, in order
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        val = np.where(inside, imgs[k][np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], 0).astype(np.int64)
        wgt = np.where(inside, np.minimum(np.minimum(sx, w - 1 - sx), np.minimum(sy, h - 1 - sy)) + 1, 0)
        first = np.where(inside & (cnt == 0), val, first)
        acc, wsum, cnt = acc + (wgt if blend == 2 else inside) * val, wsum + wgt, cnt + inside
    with np.errstate(all="ignore"):
        value = (first, acc / cnt, acc / wsum)[blend]
    want = np.where(cnt > 0, value, fill).astype(np.float32)
    assert cnt.max() >= min(w * h, 2)   # the jobs overlap
    assert out[0].tobytes() == want.tobytes() and (count[0] == cnt).all()
    assert (out[1] == fill).all() and not count[1].any()   # the empty group


@pytest.mark.parametrize("blend", [0, 1, 2])
def test_host_loop_against_float64(blend):
    """Three jobs (rot30, projective, sign_change) of one canvas.  Per job, as test_warp_host.py derives: du = 2^-22 (Sx + |u| Sw) /
    |W|, dv likewise, and the job's value moves by at most e_j = G (du_j + dv_j) + 2^-21 max|img|.  Carried through the blend:
    first: e of the first covering job; mean: sum e_j / n; feather: sum wgt_j e_j / wsum for the values, plus the weights' own
    movement - wgt is a min of u, (w - 1) - u, v, (h - 1) - v plus one, so it moves by at most du_j + dv_j and two roundings,
    2^-22 wgt_j, and a weighted mean whose weights move by dw_j moves by at most range(img) sum dw_j / wsum.  The n ordered adds
    and the division add (n + 3) 2^-24 max|img|.  Pixels within du, dv of a coverage edge of any job are left out: the union of
    three shares test_warp_host.py holds to 0.01 each on these inputs."""
    imgs = np.stack([_img(*SRC, seed=3 + k) for k in range(3)])
    models = np.array(list(GENERAL.values()), np.float32)
    out, count = CR.host(imgs, models, None, None, OUT[::-1], (0, 0), -1.0, 1, blend)
    value, cnt, wsum, jobs = CR.blend64(imgs, models, OUT[::-1], blend)
    big, G = float(abs(imgs).max()), max(abs(np.diff(imgs.astype(np.float64), axis=1)).max(), abs(np.diff(imgs.astype(np.float64), axis=2)).max())
    near, e, d = np.zeros(OUT[::-1], bool), [], []
    with np.errstate(all="ignore"):
        for r in jobs:
            du = 2.0 ** -22 * (r["Sx"] + abs(r["u"]) * r["Sw"]) / abs(r["W"])
            dv = 2.0 ** -22 * (r["Sy"] + abs(r["v"]) * r["Sw"]) / abs(r["W"])
            near |= (abs(r["W"]) < 2.0 ** -10) | ~np.isfinite(du + dv)
            for c, dc, hi in ((r["u"], du, SRC[0] - 1), (r["v"], dv, SRC[1] - 1)):
                near |= (abs(c) <= dc) | (abs(c - hi) <= dc)
            d.append(np.where(r["covered"], du + dv, 0.0))
            e.append(np.where(r["covered"], G * (du + dv) + 2.0 ** -21 * big, 0.0))
        if blend == 0:
            tol = sum(np.where(r["covered"] & (sum(q["covered"] for q in jobs[:k]) == 0), e[k], 0.0) for k, r in enumerate(jobs))
        elif blend == 1:
            tol = sum(e) / cnt
        else:
            tol = sum(r["wgt"] * e[k] for k, r in enumerate(jobs)) / wsum
            tol = tol + float(imgs.max() - imgs.min()) * sum(d[k] + 2.0 ** -22 * r["wgt"] for k, r in enumerate(jobs)) / wsum
        tol = tol + (cnt + 3) * 2.0 ** -24 * big
    assert near.mean() <= 0.03, near.mean()
    keep = ~near
    assert (count[0][keep] == cnt[keep]).all() and (cnt[keep] >= 2).mean() > 0.1   # the jobs overlap
    sel = keep & (cnt > 0)
    err = abs(out[0].astype(np.float64) - value)
    print(CR.BLENDS[blend], "left out", int(near.sum()), "max err", err[sel].max(), "min slack", (tol - err)[sel].min())
    assert (err[sel] <= tol[sel]).all()
    assert (out[0][keep & (cnt == 0)] == -1.0).all()
