"""kernels_twoband.hip against the host loop (tests/twoband_ref.py), bitwise, value and count: radii from none to a halo larger
than the canvas, both taps, both paths, with and without gains, partial tiles and an empty group; the visit counters, crop
invariance, the memory kinds and Sift.mosaic(blend="twoband") against the call it composes."""
import functools

import numpy as np
import pytest

import twoband_ref as TR
import warp_ref as WR
from sift_amd import _lib
from sift_amd.sift import Sift, pinned_array
from test_twoband_host import GAINS, OFFSETS, crop_case, gauss

pytestmark = pytest.mark.gpu
ORIGIN = (-2, 1)
INTERP = ("nearest", "bilinear")


@functools.lru_cache(maxsize=None)
def _case(w, h, ow, oh, radius, interp, gains):
    """test_composite_gpu.py's case - two images, the eight models of WR.job_models on alternating images in three groups, the
    middle one empty - with Gaussian taps of the radius, and the host loop's result (computed once)."""
    imgs = (np.random.default_rng(w + 31 * h).random((2, h, w)) * 255).astype(np.float32)
    models, src, taps = WR.job_models(w, h, ow, oh), np.arange(8, dtype=np.int32) % 2, gauss(radius, max(radius / 3.0, 0.5))
    return imgs, models, src, taps, TR.host(imgs, models, taps, OFFSETS, src, (oh, ow), ORIGIN, -1.0, interp, GAINS if gains else None)


@pytest.mark.parametrize("gains", [False, True])
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("radius", [0, 1, 3, 16])
@pytest.mark.parametrize("w,h,ow,oh", [(1, 1, 1, 1), (5, 3, 7, 2), (65, 17, 63, 33), (130, 70, 129, 49)])
def test_kernel_equals_host(ctx, w, h, ow, oh, radius, interp, path, gains):
    imgs, models, src, taps, (want, want_count) = _case(w, h, ow, oh, radius, interp, gains)
    got, count = ctx.composite_twoband(imgs, models, OFFSETS, src, (oh, ow), ORIGIN, -1.0, INTERP[interp], taps=taps, path=path, count=True,
                                       gains=GAINS if gains else None)
    assert got.tobytes() == want.tobytes() and count.tobytes() == want_count.tobytes()
    assert (got[1] == -1.0).all() and not count[1].any() and (w < 64 or count[0].max() >= 3)


def test_visit_counters(ctx):
    """A 129 x 49 canvas, one job, R = 3.  On a 240 x 112 image with the canvas at (3, 3) the identity covers every tile's whole
    window, partial tiles included (lattice points 0 .. 197 by 0 .. 69): every visit takes the constant-norm path, or the general
    one when it is forced.  Shifted by 1000 pixels no pixel is covered."""
    n = -(-129 // _lib.TWOBAND_TILE[0]) * -(-49 // _lib.TWOBAND_TILE[1])
    imgs = (np.random.default_rng(5).random((1, 112, 240)) * 255).astype(np.float32)
    visits = lambda model, path: ctx.composite_twoband(imgs, [model], out_shape=(49, 129), origin=(3, 3), taps=gauss(3, 1.0), path=path, want_tiles=True)[1]
    assert visits(WR.translation(0, 0), 0) == (0, n, 0)
    assert visits(WR.translation(0, 0), 1) == (n, 0, 0)
    assert visits(WR.translation(1000, 0), 0) == (0, 0, n)


def test_crop_invariance(ctx):
    """test_twoband_host.py's two canvases through the kernel; the crop's origin is no multiple of the tile size."""
    imgs, models, src, taps, gains, big, small, where = crop_case()
    out, count = ctx.composite_twoband(imgs, models, OFFSETS, src, fill=-1.0, taps=taps, count=True, gains=gains, **big)
    sub, sub_count = ctx.composite_twoband(imgs, models, OFFSETS, src, fill=-1.0, taps=taps, count=True, gains=gains, **small)
    assert sub.tobytes() == np.ascontiguousarray(out[(slice(None),) + where]).tobytes()
    assert sub_count.tobytes() == np.ascontiguousarray(count[(slice(None),) + where]).tobytes()
    assert sub.tobytes() == TR.host(imgs, models, taps, OFFSETS, src, fill=-1.0, gains=gains, **small)[0].tobytes()


def test_memory_kinds(ctx):
    import torch
    imgs, models, src, taps, (want, want_count) = _case(65, 17, 63, 33, 3, 1, True)
    kw = dict(offsets=OFFSETS, src=src, out_shape=(33, 63), origin=ORIGIN, fill=-1.0, taps=taps)
    out, count, mdl, gain = pinned_array(want.shape), pinned_array(want.shape, np.uint16), pinned_array(models.shape), pinned_array((8,))
    mdl[:], gain[:] = models, GAINS
    assert ctx.composite_twoband(imgs, mdl, out=out, count=count, gains=gain, **kw)[0] is out
    assert out.tobytes() == want.tobytes() and count.tobytes() == want_count.tobytes()
    d_out, d_count = torch.zeros(want.shape, dtype=torch.float32, device="cuda"), torch.zeros(want.shape, dtype=torch.int16, device="cuda")
    d_imgs, d_mdl, d_gain = torch.from_numpy(imgs).cuda(), torch.from_numpy(models).cuda(), torch.tensor(GAINS, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    ctx.composite_twoband(d_imgs, d_mdl, out=d_out, count=d_count, gains=d_gain, **kw)
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_count.cpu().numpy().tobytes() == want_count.tobytes()


@pytest.mark.parametrize("gain", [False, True])
def test_mosaic_is_the_composition(ctx, gain):
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:8 + 256])])
    sift = Sift(context=ctx)
    got = sift.mosaic(imgs, refine=2, blend="twoband", band_sigma=2.0, gain=gain)
    models, canvas, count, origin = got[:4]
    points = [sift.calculate(img) for img in imgs]
    want = sift.verify(points[0], points[1], refine=2)[1]
    jobs = np.array([WR.translation(0, 0), want["h"]], np.float32)
    gains = ctx.overlap_stats(imgs, jobs, None, [0, 1], canvas.shape, origin, gains=True)[1] if gain else None
    out, cover = ctx.composite_twoband(imgs, jobs, None, [0, 1], canvas.shape, origin, sigma=2.0, count=True, gains=gains)
    assert models[0].tobytes() == want.tobytes() and want["iteration"] >= 0
    assert canvas.tobytes() == out[0].tobytes() and count.tobytes() == cover[0].tobytes()
    assert canvas.shape[1] >= 264 and (count == 2).mean() > 0.5
    assert not gain or got[4].tobytes() == gains.tobytes()
    with pytest.raises(ValueError):
        ctx.band_taps(6.0)   # a radius of three sigma: above 16
