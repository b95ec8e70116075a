"""kernels_align.hip against the host loop (tests/align_ref.py), bitwise: both paths, partial and several tiles, the convergence
fixture, the memory kinds and Sift.register(align=) against the calls it composes."""
import functools
import math

import numpy as np
import pytest

import align_ref as A
import warp_ref as WR
from sift_amd import _lib
from sift_amd.sift import Sift, pinned_array

pytestmark = pytest.mark.gpu
KW = dict(border=1, min_pixels=16)


@functools.lru_cache(maxsize=None)
def _case(w, h, rounds):
    """A frame of the analytic image and the same image 0.7 pixels off at another exposure; six pairs: the identity, half a
    pixel, 5 degrees, a perspective model, a model that covers one corner only and the null model (computed once)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    imgs = np.stack([A.analytic(x, y), 0.8 * A.analytic(x + 0.7, y - 0.4) + 10]).astype(np.float32)
    rot = WR.rotation(5.0, 1.0, (w, h), (w, h))
    models = A.records([WR.translation(0, 0), WR.translation(0.5, 0.5), rot, WR.projective(rot, 0.02 / w, -0.01 / h),
                        WR.translation(0.75 * w, 0.75 * h), [0] * 9])
    models["iteration"][5], models["inliers"] = -1, 7
    pairs = [(0, 1)] * 3 + [(1, 0)] * 3
    return imgs, pairs, models, A.host(imgs, pairs, models, rounds, **KW)


def _same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("rounds", [0, 3])
@pytest.mark.parametrize("w,h", [(8, 8), (64, 64), (65, 67), (130, 70)])
def test_kernel_equals_host(ctx, w, h, rounds, path):
    imgs, pairs, models, want = _case(w, h, rounds)
    got = ctx.align_homography(imgs, pairs, models, rounds, path=path, want_sums=True, **KW)
    assert _same(got, want)
    out = got[1]
    assert out["status"][5] == _lib.ALIGN_NO_MODEL and (got[0]["inliers"] == 7).all()
    assert (out["rounds"][:4] == rounds).all() and (rounds or out["pixels"][0] == (w - 2) * (h - 2))


def test_convergence_fixture(ctx):
    models = A.records([A.H_START])
    got = ctx.align_homography(A.fixture(), [(0, 1)], models, 8, want_sums=True)
    assert _same(got, A.host(A.fixture(), [(0, 1)], models, 8))
    assert A.corner_error(got[1]["h"][0], A.H_TRUE, A.W, A.H) < 0.05


def test_memory_kinds(ctx):
    import torch
    imgs, pairs, models, want = _case(65, 67, 3)
    mdl, out = pinned_array(models.shape, _lib.HOMOGRAPHY_DTYPE), pinned_array(models.shape, _lib.ALIGNMENT_DTYPE)
    mdl[:] = models
    assert ctx.align_homography(imgs, pairs, mdl.ctypes.data, 3, out=out, **KW)[1] is out   # an address: rewritten in place
    assert mdl.tobytes() == want[0].tobytes() and out.tobytes() == want[1].tobytes()
    d_imgs, d_mdl = torch.from_numpy(imgs).cuda(), torch.from_numpy(models.view(np.uint8)).cuda()
    d_out = torch.zeros(want[1].nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.align_homography(d_imgs, pairs, d_mdl, 3, out=d_out, **KW)
    assert d_mdl.cpu().numpy().tobytes() == want[0].tobytes() and d_out.cpu().numpy().tobytes() == want[1].tobytes()


def test_register_and_mosaic_are_the_composition(ctx):
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:8 + 256])])
    sift, pairs = Sift(context=ctx), [(0, 1), (1, 0)]
    points = [sift.calculate(img) for img in imgs]
    verified = np.array([sift.verify(points[q], points[t], refine=2)[1] for q, t in pairs])
    assert sift.register(imgs, pairs, refine=2, align=0)[0].tobytes() == verified.tobytes()
    models, reg, mask = sift.register(imgs, pairs, refine=2, align=2)
    want, res = ctx.align_homography(imgs, pairs, verified, 2)
    assert _same((models, reg, mask), (want,) + ctx.warp_homography(imgs, want, [1, 0], mask=True))
    assert (res["status"] != _lib.ALIGN_NO_MODEL).all() and (res["rms"] <= res["rms0"]).all() and math.isfinite(res["rms"].max())
    assert want["h"].tobytes() != verified["h"].tobytes()   # a step was taken: align=2 is not align=0
    canvas = ((-4, 0), (192, 272))
    got = sift.mosaic(imgs, refine=2, align=2, canvas=canvas)
    jobs = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], want["h"][0]], np.float32)
    assert got[0].tobytes() == want[:1].tobytes()
    assert _same(got[1:3], [a[0] for a in ctx.composite_homography(imgs, jobs, None, [0, 1], canvas[1], canvas[0], 0.0, "bilinear", "feather", count=True)])
