"""kernels_warp.hip against the host loop (tests/warp_ref.py), bitwise: both paths, partial tiles and boxes, the tile counters, the
memory kinds and Sift.register against the calls it composes."""
import functools

import numpy as np
import pytest

import warp_ref as WR
from sift_amd.sift import Sift, pinned_array

pytestmark = pytest.mark.gpu
ORIGIN = (-2, 1)


@functools.lru_cache(maxsize=None)
def _case(w, h, ow, oh, interp):
    """Two images, the eight models of WR.job_models on alternating images, and the host loop's result (computed once)."""
    imgs = (np.random.default_rng(w + 31 * h).random((2, h, w)) * 255).astype(np.float32)
    models, src = WR.job_models(w, h, ow, oh), np.arange(8, dtype=np.int32) % 2
    return imgs, models, src, WR.host(imgs, models, src, (oh, ow), ORIGIN, -1.0, interp)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h,ow,oh", [(1, 1, 1, 1), (5, 3, 7, 2), (64, 16, 64, 16), (65, 17, 63, 33), (130, 70, 129, 49)])
def test_kernel_equals_host(ctx, w, h, ow, oh, interp, path):
    imgs, models, src, (want, want_mask) = _case(w, h, ow, oh, interp)
    got, mask = ctx.warp_homography(imgs, models, src, (oh, ow), ORIGIN, -1.0, ("nearest", "bilinear")[interp], path, mask=True)
    assert got.tobytes() == want.tobytes() and mask.tobytes() == want_mask.tobytes()
    assert w < 64 or (mask[:4].any(axis=(1, 2)).all() and not mask[6:].any())


def test_tile_counters(ctx):
    """129 x 49 is 3 x 4 tiles.  The identity's boxes are 68 x 20 floats; the first tile of the minification by 8 maps to 505 x
    121 source pixels, which clipped to the 130 x 70 image is 131 * 70 floats: above the 8192 of the LDS budget."""
    imgs, models, _, _ = _case(130, 70, 129, 49, 1)
    count = lambda job, path: ctx.warp_homography(imgs[:1], models[job:job + 1], None, (49, 129), path=path, want_tiles=True)[1]
    assert count(0, 0) == (12, 0)
    staged, direct = count(4, 0)
    assert direct >= 1 and staged + direct == 12
    assert count(0, 1) == (0, 12)


def test_memory_kinds(ctx):
    import torch
    imgs, models, src, (want, want_mask) = _case(65, 17, 63, 33, 1)
    kw = dict(src=src, out_shape=(33, 63), origin=ORIGIN, fill=-1.0, mask=None)
    out, mask, mdl = pinned_array(want.shape), pinned_array(want.shape, np.uint8), pinned_array(models.shape)
    mdl[:] = models
    assert ctx.warp_homography(imgs, mdl, out=out, **dict(kw, mask=mask))[0] is out
    assert out.tobytes() == want.tobytes() and mask.tobytes() == want_mask.tobytes()
    d_out, d_mask = torch.zeros(want.shape, dtype=torch.float32, device="cuda"), torch.zeros(want.shape, dtype=torch.uint8, device="cuda")
    d_imgs, d_mdl = torch.from_numpy(imgs).cuda(), torch.from_numpy(models).cuda()
    torch.cuda.synchronize()
    ctx.warp_homography(d_imgs, d_mdl, out=d_out, **dict(kw, mask=d_mask))
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_mask.cpu().numpy().tobytes() == want_mask.tobytes()


def test_register_is_the_composition(ctx):
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:8 + 256])])
    sift = Sift(context=ctx)
    models, reg, mask = sift.register(imgs, [(0, 1), (1, 0)], refine=2)
    points = [sift.calculate(img) for img in imgs]
    want = np.array([sift.verify(points[q], points[t], refine=2)[1] for q, t in ((0, 1), (1, 0))])
    out, cover = ctx.warp_homography(imgs, want, [1, 0], mask=True)
    assert models.tobytes() == want.tobytes() and reg.tobytes() == out.tobytes() and mask.tobytes() == cover.tobytes()
    assert (models["iteration"] >= 0).all() and (mask.mean(axis=(1, 2)) > 0.5).all()
