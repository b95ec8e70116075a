"""kernels_localize.hip against the host loop (tests/localize_ref.py) and the `use` switch against the generic calls: all bitwise."""
import functools
import os

import numpy as np
import pytest

import localize_ref as LR
from sift_amd import _lib
from sift_amd.sift import Context, K_SQRT2

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _points_case(L, w, h, m, quad):
    rng = np.random.default_rng(1000 * L + w + m)
    if quad:   # an exact quadratic with a flat patch and a NaN: finished lanes, movers of one to three moves, every status, in one wave
        stack = LR.quadratic_stack(L, w, h, (30, 4, 2), (0.25, -0.375, 0.125))
        stack[:, 1:6, 50:55], stack[2, 4, 10] = 7.0, np.nan
        pts = np.resize(np.array([[30, 4, 2], [29, 4, 2], [28, 4, 2], [27, 4, 2], [30, 3, 2], [30, 4, 1], [52, 3, 2], [10, 4, 2], [11, 5, 2], [65, 4, 2], [33, 5, 3]]), (m, 3))
        return stack, pts[:, 0], pts[:, 1], pts[:, 2]
    stack = (rng.random((L, h, w)) * 64 + 96).astype(np.float32)
    xs, ys, idx = rng.integers(1, w - 1, m), rng.integers(1, h - 1, m), rng.integers(1, L - 1, m)
    for k, (x, y) in enumerate([(1, 2), (w - 2, 2), (3, 1), (3, h - 2)][:m]):   # the first points sit on the four borders of the interior
        xs[k], ys[k] = x, y
    return stack, xs, ys, idx


@pytest.mark.parametrize("max_moves", [0, 1, 5])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("L,w,h,quad", [(3, 8, 8, 0), (5, 8, 8, 0), (3, 67, 9, 0), (5, 67, 9, 0), (5, 67, 9, 1)])
def test_points_equal_host(ctx, L, w, h, quad, m, max_moves):
    stack, xs, ys, idx = _points_case(L, w, h, m, quad)
    got = ctx.localize_points(stack, xs, ys, idx, max_moves)
    assert LR.same(got, LR.host(stack, xs, ys, idx, max_moves))
    if quad and m >= 63:
        assert {0, 1, 2, 4} <= set(got["status"])   # the point 35 samples from the vertex never converges within 8 moves
        assert max_moves < 5 or (got["moves"][3], got["mx"][3], got["x"][3], got["dy"][3]) == (3, 3, 30.25, -0.375)


def _crops(width):
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    return np.stack([np.ascontiguousarray(big[:, 0:width]), np.ascontiguousarray(big[:, 8:8 + width])])


@pytest.mark.parametrize("dogs", [3, 5])
@pytest.mark.parametrize("subpixel", [0, 1])
@pytest.mark.parametrize("width", [256, 250])   # Gaussian levels only / rows not 16-byte aligned: DoG levels written
def test_batch_equals_host(ctx, width, subpixel, dogs):
    params = _lib.Params(dogs, 3 if dogs == 3 else 1, 1.6, K_SQRT2, subpixel)   # five DoGs: one octave, where no dead 16 x 16 blur throws
    ctx.calculate_batch(_crops(width), params)
    got, kp = ctx.localize(), ctx.results()[0]
    assert kp.size > 50 and LR.same(got, LR.batch_host(ctx, dogs, subpixel)) and (got["status"] == LR.OK).any() and (got["moves"] > 0).any()
    assert dogs == 3 or set(kp["index"]) == {1, 2, 3}


def test_thrown_image_and_out_memory(ctx):
    import torch
    from sift_amd.sift import pinned_array
    g = np.load(os.path.join(LR.FR.ROOT, "tests", "golden", "mixed_status_frames.npz"))
    dogs, octaves, sigma, k, subpixel = g["params"].tolist()
    ctx.calculate_batch(g["frames"][[0, 1, 2]].astype(np.float32), _lib.Params(int(dogs), int(octaves), sigma, k, int(subpixel)), raise_on_error=False)
    counts = ctx.counts()
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0 and ctx.status()[1] != 0
    got, want = ctx.localize(), LR.batch_host(ctx, int(dogs), subpixel)
    assert got.size == counts.sum() and LR.same(got, want)
    pinned = pinned_array((got.size,), LR.DTYPE)
    dev = torch.zeros(got.size * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.localize(out=pinned) is pinned and LR.same(pinned, want)
    ctx.localize(out=dev)
    assert dev.cpu().numpy().tobytes() == want.tobytes()


def test_use_switch(ctx):
    params = _lib.Params(3, 3, 1.6, K_SQRT2, 0)
    imgs, pairs = _crops(256), [(0, 1), (1, 0)]
    ctx.calculate_batch(imgs, params)
    kp, desc = ctx.results()
    base = np.concatenate([[0], np.cumsum(ctx.counts())])
    loc = ctx.localize()
    fine = np.stack([loc["x"], loc["y"]], axis=1)
    plain = np.stack([(kp["x"].astype(np.int64) << kp["octave"]), (kp["y"].astype(np.int64) << kp["octave"])], axis=1).astype(np.float32)
    assert not LR.same(fine, plain)
    rec, counts = ctx.match_images(pairs, 0.8, False)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pair_of = np.repeat(np.arange(len(pairs)), counts)
    rows = np.stack([base[np.array(pairs)[pair_of, 0]] + rec["query"], base[np.array(pairs)[pair_of, 1]] + rec["train"]], axis=1)

    def check(coords, localized):
        pts = np.concatenate([coords[rows[:, 0]], coords[rows[:, 1]]], axis=1)
        for model, refine in (("homography", 0), ("homography", 2), ("fundamental", 0)):
            got = ctx.verify_images(pairs, 0.8, False, 512, 1.0, 19, refine, model, localized=localized)
            want = (ctx.ransac_fundamental if model == "fundamental" else ctx.ransac_homography)(pts, off, 512, 1.0, 19, refine=refine)
            assert LR.same(got[0], rec) and LR.same(got[2], want[0]) and LR.same(got[3], want[1]), (model, refine, localized)
        return got[2], pts

    models, pts = check(fine, True)
    got = ctx.refine_fundamental_images(pairs, rec, counts, models, 1.0, 3, localized=True)
    assert all(LR.same(a, b) for a, b in zip(got, ctx.refine_fundamental(pts, off, models, 1.0, 3)))
    hm = ctx.ransac_homography(pts, off, 512, 1.0, 19)[0]
    got = ctx.match_images_guided(pairs, hm["h"], "homography", 2.0, 0.8, True, localized=True)
    want = ctx.match_guided_sets(desc, fine, base.astype(np.int64), pairs, hm["h"], "homography", 2.0, 0.8, True, kp)
    assert LR.same(got[0], want[0]) and LR.same(got[1], want[1]) and got[0].size > 0
    ctx.calculate_batch(imgs, params)   # every calculate resets the switch
    check(plain, False)


def _points(c, L=3, x=3, y=3, i=1, max_moves=5):   # the known-answer entry on an 8 x 8 stack
    return c.localize_points(np.zeros((L, 8, 8), np.float32), [x], [y], [i], max_moves)


@pytest.mark.parametrize("call", [lambda c: c.localize(-1), lambda c: c.localize(9), lambda c: c.localize(5, 2), lambda c: Context(0).localize(), lambda c: _points(c, L=2),
                                  lambda c: _points(c, max_moves=9), lambda c: _points(c, x=0), lambda c: _points(c, x=7), lambda c: _points(c, y=0),
                                  lambda c: _points(c, y=7), lambda c: _points(c, i=0), lambda c: _points(c, i=2)])
def test_einval(ctx, call):
    ctx.calculate_batch(_crops(256)[:1], _lib.Params(3, 2, 1.6, K_SQRT2, 0))
    with pytest.raises(ValueError):   # max_moves, use, a fresh context that holds no results; then the known-answer entry's arguments
        call(ctx)


def test_cli_and_cpp_example_agree(tmp_path):
    """The CLI with --localize and examples/sift_verify.cpp with its trailing localize argument: the same H lines, the same inliers.txt."""
    import subprocess
    import sys
    from sift_amd import cli
    root, lib = LR.FR.ROOT, os.path.join(LR.FR.ROOT, "sift_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "sift_verify.cpp"),
                           "-L" + lib, "-lsift_hip", "-Wl,-rpath," + lib, "-o", str(tmp_path / "sift_verify")])
    img = cli.read_image(os.path.join(root, "tests", "golden", "parrot_r.pgm")).astype(np.uint8)
    for name, part in (("a.pgm", img[:, :-8]), ("b.pgm", img[:, 8:])):
        (tmp_path / name).write_bytes(b"P5\n%d %d\n255\n" % part.shape[::-1] + np.ascontiguousarray(part).tobytes())
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    runs = {"cpp": [str(tmp_path / "sift_verify"), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "2048", "3", "0", "2", "homography", "-1", "1"],
            "py": [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay", "--verify", "--refine", "2", "--localize"]}
    lines = {}
    for d, cmd in runs.items():
        (tmp_path / d).mkdir()
        out = subprocess.run(cmd, cwd=tmp_path / d, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        lines[d] = [ln for ln in out.stdout.splitlines() if ln.startswith("H ")]
    assert len(lines["cpp"]) == 3 and lines["cpp"] == lines["py"]
    assert (tmp_path / "cpp" / "inliers.txt").read_bytes() == (tmp_path / "py" / "inliers.txt").read_bytes()
