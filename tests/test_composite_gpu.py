"""kernels_composite.hip against the host loop (tests/composite_ref.py), bitwise, value and count: every blend, both taps and both
paths, partial tiles and boxes, an empty group, the visit counters, the memory kinds and Sift.mosaic against the calls it composes."""
import functools

import numpy as np
import pytest

import composite_ref as CR
import warp_ref as WR
from sift_amd.sift import Sift, pinned_array

pytestmark = pytest.mark.gpu
ORIGIN, OFFSETS = (-2, 1), [0, 5, 5, 8]
INTERP = ("nearest", "bilinear")


@functools.lru_cache(maxsize=None)
def _case(w, h, ow, oh, interp, blend):
    """Two images, the eight models of WR.job_models on alternating images in three groups, the middle one empty, and the host
    loop's result (computed once)."""
    imgs = (np.random.default_rng(w + 31 * h).random((2, h, w)) * 255).astype(np.float32)
    models, src = WR.job_models(w, h, ow, oh), np.arange(8, dtype=np.int32) % 2
    return imgs, models, src, CR.host(imgs, models, OFFSETS, src, (oh, ow), ORIGIN, -1.0, interp, blend)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("w,h,ow,oh", [(1, 1, 1, 1), (5, 3, 7, 2), (64, 16, 64, 16), (65, 17, 63, 33), (130, 70, 129, 49)])
def test_kernel_equals_host(ctx, w, h, ow, oh, blend, interp, path):
    imgs, models, src, (want, want_count) = _case(w, h, ow, oh, interp, blend)
    got, count = ctx.composite_homography(imgs, models, OFFSETS, src, (oh, ow), ORIGIN, -1.0, INTERP[interp], CR.BLENDS[blend], path, count=True)
    assert got.tobytes() == want.tobytes() and count.tobytes() == want_count.tobytes()
    assert (got[1] == -1.0).all() and not count[1].any() and (w < 64 or count[0].max() >= 3)


def test_visit_counters(ctx):
    """129 x 49 is 3 x 4 tiles, one job: 12 visits.  Under the identity every tile has covered pixels and a box of at most 67 x 19 floats;
    shifted by 1000 pixels no pixel is covered; under the minification by 8 only the first tile is (x <= 16, y <= 8), and its
    footprint, 131 * 70 floats after clipping, is above a buffer's 4092."""
    imgs, models, _, _ = _case(130, 70, 129, 49, 1, 2)
    visits = lambda model, path: ctx.composite_homography(imgs[:1], [model], out_shape=(49, 129), path=path, want_tiles=True)[1]
    assert visits(models[0], 0) == (12, 0, 0)
    assert visits(models[0], 1) == (0, 12, 0)
    assert visits(WR.translation(1000, 0), 0) == (0, 0, 12)
    tiles = visits(models[4], 0)
    assert tiles[1] >= 1 and sum(tiles) == 12


def test_memory_kinds(ctx):
    import torch
    imgs, models, src, (want, want_count) = _case(65, 17, 63, 33, 1, 2)
    kw = dict(offsets=OFFSETS, src=src, out_shape=(33, 63), origin=ORIGIN, fill=-1.0)
    out, count, mdl = pinned_array(want.shape), pinned_array(want.shape, np.uint16), pinned_array(models.shape)
    mdl[:] = models
    assert ctx.composite_homography(imgs, mdl, out=out, count=count, **kw)[0] is out
    assert out.tobytes() == want.tobytes() and count.tobytes() == want_count.tobytes()
    d_out, d_count = torch.zeros(want.shape, dtype=torch.float32, device="cuda"), torch.zeros(want.shape, dtype=torch.int16, device="cuda")
    d_imgs, d_mdl = torch.from_numpy(imgs).cuda(), torch.from_numpy(models).cuda()
    torch.cuda.synchronize()
    ctx.composite_homography(d_imgs, d_mdl, out=d_out, count=d_count, **kw)
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_count.cpu().numpy().tobytes() == want_count.tobytes()


def test_mosaic_is_the_composition(ctx):
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:8 + 256])])
    sift = Sift(context=ctx)
    models, canvas, count, origin = sift.mosaic(imgs, refine=2)
    points = [sift.calculate(img) for img in imgs]
    want = sift.verify(points[0], points[1], refine=2)[1]
    jobs = np.array([WR.translation(0, 0), want["h"]], np.float32)
    out, cover = ctx.composite_homography(imgs, jobs, None, [0, 1], canvas.shape, origin, count=True)
    assert models[0].tobytes() == want.tobytes() and want["iteration"] >= 0
    assert canvas.tobytes() == out[0].tobytes() and count.tobytes() == cover[0].tobytes()
    assert canvas.shape[1] >= 264 and (count == 2).mean() > 0.5
