"""kernels_overlap.hip against the host loop (tests/overlap_ref.py), bytewise: statistics, gains and status for both paths and taps,
partial chunks, several regions, 32 live jobs, the int32 extremes; the compositor with gains; Sift.mosaic(gain=True)."""
import functools

import numpy as np
import pytest

import composite_ref as CR
import overlap_ref as OR
import warp_ref as WR
from sift_amd.sift import Sift

pytestmark = pytest.mark.gpu
INTERP = ("nearest", "bilinear")


# (130, 70, 129, 49): partial chunks and regions; (70, 150, 150, 140): 3 x 3 regions, accumulators kept across 16 chunks
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("w,h,ow,oh", OR.SHAPES + [(130, 70, 129, 49), (70, 150, 150, 140)])
def test_kernel_equals_host(ctx, w, h, ow, oh, interp, path):
    imgs, models, src, want = OR.case(w, h, ow, oh, interp)
    got = ctx.overlap_stats(imgs, models, OR.OFFSETS, src, (oh, ow), OR.ORIGIN, 1.0, INTERP[interp], gains=True, path=path)
    for g, r in zip(got, want):
        assert g.tobytes() == r.tobytes()
    assert not got[0][1].any() and (w < 64 or got[0][0, 0, 0, 1] > 0)


@functools.lru_cache(maxsize=None)
def _many():
    imgs = (np.random.default_rng(5).random((2, 40, 48)) * 255).astype(np.float32)
    models = np.array([WR.translation(k % 7 - 3, k // 7 - 2) for k in range(33)], np.float32)
    return imgs, models, np.arange(33, dtype=np.int32) % 2


def test_32_jobs_and_the_limit(ctx):
    imgs, models, src = _many()
    want = OR.host(imgs, models[:32], None, src[:32], (45, 70), (-3, -2))
    got = ctx.overlap_stats(imgs, models[:32], None, src[:32], (45, 70), (-3, -2), gains=True)
    for g, r in zip(got, want):
        assert g.tobytes() == r.tobytes()
    assert (got[0][0, 0] > 0).all()
    with pytest.raises(ValueError, match="more than 32 jobs"):   # SIFT_HIP_EINVAL
        ctx.overlap_stats(imgs, models, None, src, (45, 70))


@pytest.mark.parametrize("level", [0.0, 255.0])
def test_int32_extremes(ctx, level):
    """One region fully covered by two identity jobs: with q = 0 every product of the offset planes is +2^14, 2^26 a region."""
    stats = ctx.overlap_stats(np.full((1, 64, 64), level, np.float32), [WR.translation(0, 0)] * 2, src=[0, 0])
    px, q = 64 * 64, int(level)
    for k, v in enumerate((px, q * px, q * q * px, q * q * px)):
        assert (stats[0, k, :2, :2] == v).all()
    assert stats.sum() == 4 * px * (1 + q + 2 * q * q)


@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("device", [False, True])
def test_composite_with_gains(ctx, blend, device):
    imgs, models, src, _ = OR.case(130, 70, 129, 49, 1)
    gains = np.linspace(0.7, 1.4, 8).astype(np.float32)
    want, want_count = OR.host_composite(imgs, models, gains, OR.OFFSETS, src, (49, 129), OR.ORIGIN, -1.0, 1, blend)
    g = gains
    if device:
        import torch
        g = torch.from_numpy(gains).cuda()
        torch.cuda.synchronize()
    got, count = ctx.composite_homography(imgs, models, OR.OFFSETS, src, (49, 129), OR.ORIGIN, -1.0, "bilinear", CR.BLENDS[blend], count=True, gains=g)
    assert got.tobytes() == want.tobytes() and count.tobytes() == want_count.tobytes()


def test_zncc_of_the_exposure_fixture(ctx):
    """Translated cuts of one picture correlate near 1 whatever their exposure."""
    imgs, models, shape = OR.exposure_fixture()
    stats, gains, status = ctx.overlap_stats(imgs, models, out_shape=shape, gains=True)
    want = OR.host(imgs, models, None, None, shape)
    assert stats.tobytes() == want[0].tobytes() and gains.tobytes() == want[1].tobytes() and not status.any()
    zncc = ctx.overlap_zncc(stats[0], 3)[np.triu_indices(3, 1)]
    print("zncc", zncc, "numpy", ctx.overlap_zncc(OR.numpy_stats(imgs, models, None, shape), 3)[np.triu_indices(3, 1)])
    assert (zncc > 0.9).all()


def test_mosaic_with_gain_is_the_composition(ctx):
    """test_composite_gpu's two frames (SIFT cannot register the 96 x 64 frames of the exposure fixture), exposed 1 and 1.25"""
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:8 + 256]) * np.float32(1.25)])
    sift = Sift(context=ctx)
    found, pic, count, origin, gains, zncc = sift.mosaic(imgs, refine=2, gain=True)
    jobs = np.array([WR.translation(0, 0), found[0]["h"]], np.float32)
    stats, want_gains, status = ctx.overlap_stats(imgs, jobs, None, [0, 1], pic.shape, origin, gains=True)
    out, cover = ctx.composite_homography(imgs, jobs, None, [0, 1], pic.shape, origin, count=True, gains=want_gains)
    print("gains", gains, "zncc", zncc[0, 1])
    assert found[0]["iteration"] >= 0 and not status.any() and gains[0] > gains[1]
    assert gains.tobytes() == want_gains.tobytes() and pic.tobytes() == out[0].tobytes() and count.tobytes() == cover[0].tobytes()
    assert np.array_equal(zncc, ctx.overlap_zncc(stats[0], 2), equal_nan=True)
    plain = sift.mosaic(imgs, refine=2)
    assert len(plain) == 4 and plain[2].tobytes() == count.tobytes() and plain[1].tobytes() != pic.tobytes()
