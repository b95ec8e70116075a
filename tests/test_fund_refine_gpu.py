"""The GPU refit of F (ransac_fund_refine_kernel behind sift_hip_refine_fundamental and sift_hip_result_refine_fundamental)
against the host loop (tests/fund_refine_ref.py: hostmath_refine_fundamental, sift_amd/csrc/ransac_fund_refine_math.h in plain
loops, itself checked by tests/test_fund_refine_host.py).  Every comparison is bitwise: the records, `refined` and the flags."""
import functools

import numpy as np
import pytest

import fund_ref as FR
import fund_refine_ref as G
from sift_amd import _lib

pytestmark = pytest.mark.gpu

STAGED = 2048   # kFundRefineRows (sift_amd/csrc/ransac_kernels.h): the rows of a set that stay in LDS
# below the eight inliers of a round, the 256 partials (less than one, one, more than one row a lane), both row paths, and a
# set past the 64 x 256 rows of the lanes' inlier masks
SET_SIZES = [7, 8, 9, 255, 256, 257, 513, STAGED, STAGED + 1, 16384 + 300]
THR = 3.0


@functools.lru_cache(maxsize=None)
def _case(m):
    """m noisy rows and a deliberately poor start (the model of eight of them, of seven for m = 7) with the checker's result."""
    if m >= 8:
        rows, _, start = G.noisy_case(m, m)
    else:
        rows = G.noisy_case(m, 8)[0][:m]
        start = G.model_of(FR.numpy_models(rows)[0], 2, 1)
    return rows, start, {r: G.refine(rows, start, None, THR, r) for r in (0, 1, 3, 8)}


def _same(got, want, what=""):
    assert np.asarray(got[0]).tobytes() == want[0].tobytes(), (what, got[0], want[0])
    assert FR.same_bits(np.asarray(got[1]), want[1]) and FR.same_bits(np.asarray(got[2]), want[2]), (what, got[1], want[1])


@pytest.mark.parametrize("rounds", [0, 1, 3, 8])
@pytest.mark.parametrize("m", SET_SIZES)
def test_single_sets(ctx, m, rounds):
    rows, start, want = _case(m)
    _same(ctx.refine_fundamental(rows, None, start, THR, rounds), want[rounds], (m, rounds))
    assert want[rounds][1][0] <= rounds and want[rounds][0]["inliers"][0] >= want[0][0]["inliers"][0]


def _nine_sets():
    rng = np.random.default_rng(90)
    planar = np.concatenate([rng.random((150, 2)) * 1000] * 2, axis=1) + [0, 0, 12.5, -7.25]   # a pure shift: F is not determined
    bad = _case(257)[0].copy()
    bad[[3, 77, 130], [0, 3, 1]] = [np.nan, np.inf, -np.inf]
    bad[131] = np.nan
    parts = [_case(513)[0], np.zeros((0, 4)), _case(7)[0], _case(256)[0], planar, bad, _case(STAGED + 1)[0], _case(9)[0], _case(255)[0]]
    start = np.concatenate([_case(513)[1], _case(8)[1], _case(7)[1], _case(256)[1], G.model_of([[0, 0, -7.25], [0, 0, -12.5], [7.25, 12.5, 0]]),
                            _case(257)[1], _case(STAGED + 1)[1], _case(9)[1], _case(255)[1]])
    start["iteration"][3] = -1
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(np.float32), off, start


def test_nine_sets_one_call(ctx):
    """An empty set, a seven-row set, a model that is none, a planar set under a model of its shift, a set with non-finite rows."""
    pts, off, start = _nine_sets()
    for rounds in (0, 2, 8):
        want = G.refine(pts, start, off, THR, rounds)
        _same(ctx.refine_fundamental(pts, off, start, THR, rounds), want, rounds)
    models, refined, flags = want
    assert models[3:4].tobytes() == start[3:4].tobytes() and refined[[1, 2, 3]].tolist() == [0, 0, 0] and not flags[off[3]:off[4]].any()
    assert refined[[0, 5]].min() >= 1 and refined.max() >= 2 and models["inliers"][4] == 150 and models["inliers"][1] == 0
    assert FR.same_bits(models["iteration"], start["iteration"]) and FR.same_bits(models["root"], start["root"])


def test_pointer_kinds(ctx):
    """Page-locked and device memory for the rows, the models, `refined` and the flags: the bytes of the pageable call."""
    import torch
    from sift_amd.sift import pinned_array
    pts, off, start = _nine_sets()
    want = G.refine(pts, start, off, THR, 3)
    ppts, pm = pinned_array(pts.shape, np.float32), pinned_array((9,), _lib.FUNDAMENTAL_DTYPE)
    pr, pf = pinned_array((9,), np.int32), pinned_array((pts.shape[0],), np.uint8)
    ppts[...], pm[...], pr[...], pf[...] = pts, start.view(_lib.FUNDAMENTAL_DTYPE), 7, 9
    ctx.refine_fundamental(ppts, off, int(pm.ctypes.data), THR, 3, refined_out=pr, inlier_out=pf)
    _same((pm, pr, pf), want)
    dpts = torch.from_numpy(pts).cuda()
    dm = torch.from_numpy(start.view(np.int32).reshape(9, 12).copy()).cuda()
    dr = torch.full((9,), 7, dtype=torch.int32, device="cuda")
    df = torch.full((pts.shape[0],), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.refine_fundamental(dpts, off, dm, THR, 3, refined_out=dr, inlier_out=df)
    _same((dm.cpu().numpy(), dr.cpu().numpy(), df.cpu().numpy()), want)
    _same(ctx.refine_fundamental(dpts, off, start, THR, 3), want)   # rows on the device, the rest in host memory


@pytest.mark.parametrize("bad", [dict(rounds=9), dict(rounds=-1), dict(threshold=0.0), dict(threshold=float("nan")),
                                 dict(threshold=float("inf")), dict(offsets=[0, 5, 3]), dict(offsets=[-1, 9])])
def test_einval(ctx, bad):
    rows, start, _ = _case(9)
    args = dict(offsets=None, threshold=THR, rounds=2)
    args.update(bad)
    models = np.concatenate([start] * (len(args["offsets"]) - 1)) if args["offsets"] else start
    with pytest.raises(ValueError):
        ctx.refine_fundamental(rows, args["offsets"], models, args["threshold"], args["rounds"])


def test_result_refine_real_batch():
    """The two crops of test_result_verify_fundamental_real_batch: sift_hip_result_refine_fundamental on the records and models
    of verify_images equals sift_hip_refine_fundamental, and the checker, on coordinates gathered in numpy."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    kp, _ = ctx.results()
    base = np.concatenate([[0], np.cumsum(ctx.counts())])
    pairs = [(0, 1), (1, 0)]
    rec, counts, models, _ = ctx.verify_images(pairs, 0.8, False, 512, 1.0, 19, model="fundamental")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.zeros((rec.size, 4), np.float32)
    for p, (a, b) in enumerate(pairs):
        r = rec[off[p]:off[p + 1]]
        for col, k in ((0, kp[base[a] + r["query"]]), (2, kp[base[b] + r["train"]])):
            pts[off[p]:off[p + 1], col] = (k["x"].astype(np.int64) << k["octave"]).astype(np.float32)
            pts[off[p]:off[p + 1], col + 1] = (k["y"].astype(np.int64) << k["octave"]).astype(np.float32)
    for rounds in (0, 8):
        got = ctx.refine_fundamental_images(pairs, rec, counts, models, 1.0, rounds)
        _same(got, G.refine(pts, models, off, 1.0, rounds), rounds)
        _same(got, ctx.refine_fundamental(pts, off, models, 1.0, rounds), rounds)
    assert (got[0]["inliers"] >= models["inliers"]).all()
    spoiled = rec.copy()
    spoiled["train"][5] = 1 << 20
    with pytest.raises(ValueError):
        ctx.refine_fundamental_images(pairs, spoiled, counts, models, 1.0, 1)
    ctx.close()


def test_cli_and_cpp_example_agree(tmp_path):
    """`python -m sift_amd.cli ... --verify --model fundamental --refit 3` and examples/sift_verify.cpp with its trailing refit
    count (sift::Matcher::refine_fundamental): the same F and `refitted` line, the same inliers.txt byte for byte; --refit
    without the fundamental model is an error."""
    import os
    import subprocess
    import sys
    from sift_amd import cli
    root = FR.ROOT
    exe = tmp_path / "sift_verify"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_verify.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    img = cli.read_image(os.path.join(root, "tests", "golden", "parrot_r.pgm")).astype(np.uint8)
    h, w = img.shape
    for name, part in (("a.pgm", img[:, :w - 8]), ("b.pgm", img[:, 8:])):
        with open(tmp_path / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w - 8, h) + np.ascontiguousarray(part).tobytes())
    for d in ("cpp", "py"):
        (tmp_path / d).mkdir()
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "2048", "3", "0", "0", "fundamental", "3"], cwd=tmp_path / "cpp",
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    cpp_lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("F ", "refitted ")) or "inliers" in ln]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay", "--verify"]
    out = subprocess.run(base + ["--model", "fundamental", "--refit", "3"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    py_lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("F ", "refitted "))]
    assert len(py_lines) == 4 and py_lines == [ln for ln in cpp_lines if ln.startswith(("F ", "refitted "))]
    assert open(tmp_path / "cpp" / "inliers.txt", "rb").read() == open(tmp_path / "py" / "inliers.txt", "rb").read()
    out = subprocess.run(base + ["--refit", "3"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--refit needs" in out.stderr
