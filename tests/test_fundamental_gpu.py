"""GPU epipolar verification (sift_hip_ransac_fundamental / sift_hip_result_verify_fundamental) against the host loop
(tests/fund_ref.py: hostmath_ransac_fundamental, sift_amd/csrc/ransac_fund_math.h in plain loops, itself checked by
tests/test_fundamental_host.py).  Every comparison is bitwise: the model records, the flags and the score of every slot."""
import numpy as np
import pytest

import fund_ref as F
from sift_amd import _lib

pytestmark = pytest.mark.gpu

# the edges of the scoring kernel's tiles: 1024 rows of a set; 256 slots = 85 1/3 samples
SET_SIZES = [0, 6, 7, 8, 1023, 1024, 1025]
ITERATIONS = [1, 85, 86, 255, 256, 257]


def _expect(got, want, what=""):
    models, flags, scores = got
    assert F.same_bits(scores, want[2]), (what, np.argwhere(scores != want[2])[:8].tolist())
    assert models.astype(F.MODEL_DTYPE).tobytes() == want[0].tobytes(), (what, models, want[0])
    assert F.same_bits(flags, want[1]), what


def _sets(rng, sizes, gen):
    parts = [gen(rng, m) for m in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(parts).astype(np.float32).reshape(-1, 4), off


def _two_view(rng, m):
    return F.two_view_rows(rng, m, outliers=0.4)[0]


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_tile_edges(ctx, iterations):
    """Every set size at every iteration count, the sizes as the sets of one call (a set's tiles are its own)."""
    rng = np.random.default_rng(200 + iterations)
    for gen in (_two_view, F.random_rows):
        pts, off = _sets(rng, SET_SIZES, gen)
        got = ctx.ransac_fundamental(pts, off, iterations, 1.0, 5, want_scores=True)
        assert got[2].shape == (len(SET_SIZES), 3 * iterations)
        _expect(got, F.ransac(pts, off, iterations, 1.0, 5), gen.__name__)
        assert (got[0]["iteration"][:2] == -1).all() and (got[0]["root"][:2] == -1).all() and (got[2][:2] == -1).all()
        assert (got[0]["iteration"][2:] >= 0).all()
        if gen is _two_view and iterations >= 255:
            assert (got[0]["inliers"][4:] >= 400).all()   # the data's model is found: not a run of -1s


def test_many_sets_equal_each_alone(ctx):
    """A mix of sizes with empty and too short sets in one call equals every set on its own - at the same set number, which
    enters the draw: a set alone is called with its number of empty sets in front of it."""
    rng = np.random.default_rng(7)
    sizes = [65, 0, 1000, 6, 0, 257, 1025, 7, 3, 64]
    pts, off = _sets(rng, sizes, _two_view)
    models, flags, scores = ctx.ransac_fundamental(pts, off, 100, 1.0, 1, want_scores=True)
    _expect((models, flags, scores), F.ransac(pts, off, 100, 1.0, 1))
    assert [int(i) >= 0 for i in models["iteration"]] == [m >= 7 for m in sizes]
    for s, m in enumerate(sizes):
        rows = pts[off[s]:off[s + 1]]
        one = ctx.ransac_fundamental(rows, [0] * (s + 1) + [m], 100, 1.0, 1, want_scores=True)
        assert F.same_bits(one[0][s:], models[s:s + 1]) and F.same_bits(one[1], flags[off[s]:off[s + 1]])
        assert F.same_bits(one[2][s], scores[s])
    # offsets that start above 0: the rows in front belong to no set
    got = ctx.ransac_fundamental(pts, off[2:], 100, 1.0, 1, want_scores=True)
    _expect(got, F.ransac(pts, off[2:], 100, 1.0, 1))
    assert not got[1][:off[2]].any()


def test_ties_go_to_the_lowest_slot(ctx):
    """A set of seven rows twice: a sample that draws a row and its copy is invalid (the elimination cancels them exactly),
    every other sample is the same seven rows in some order and all fourteen rows are its inliers."""
    seven = F.fixed_samples(1)[0]
    pts = np.concatenate([seven, seven])
    models, flags, scores = ctx.ransac_fundamental(pts, None, 1024, 1.0, 0, want_scores=True)
    _expect((models, flags, scores), F.ransac(pts, None, 1024, 1.0, 0))
    top = np.nonzero(scores[0] == scores[0].max())[0]
    assert scores[0].max() == 14 and top.size >= 8 and (scores[0] == -1).sum() > 2048
    assert 3 * models[0]["iteration"] + models[0]["root"] == top[0] and models[0]["inliers"] == 14 == flags.sum()
    assert len({int(t) // 3 for t in top}) >= 4                   # the tie is between different samples


@pytest.mark.parametrize("m,iterations", [(40000, 3), (7, 65536)])
def test_split_independence(ctx, m, iterations):
    rng = np.random.default_rng(m)
    pts = _two_view(rng, m)
    got = ctx.ransac_fundamental(pts, None, iterations, 1.0, 2, want_scores=True)
    _expect(got, F.ransac(pts, None, iterations, 1.0, 2))
    assert got[0]["iteration"][0] >= 0


def test_bad_values_and_parameter_errors(ctx):
    rng = np.random.default_rng(9)
    pts = _two_view(rng, 400)
    bad_rows = [3, 77, 130, 131, 399]
    pts[3, 0] = np.nan
    pts[77, 3] = np.inf
    pts[130, 1] = -np.inf
    pts[131] = np.nan
    pts[399, 2] = np.inf
    got = ctx.ransac_fundamental(pts, None, 256, 1.0, 4, want_scores=True)
    _expect(got, F.ransac(pts, None, 256, 1.0, 4))
    assert not got[1][bad_rows].any() and got[0]["inliers"][0] > 100
    ok = _two_view(rng, 10)
    for kw in (dict(refine=1), dict(refine=8), dict(iterations=0), dict(iterations=65537), dict(threshold=0.0), dict(threshold=-1.0),
               dict(threshold=float("nan")), dict(threshold=float("inf"))):
        with pytest.raises(ValueError):
            ctx.ransac_fundamental(ok, None, **kw)
    for off in ([0, 6, 5, 10], [-1, 10]):
        with pytest.raises(ValueError):
            ctx.ransac_fundamental(ok, off)
    assert ctx.ransac_fundamental(ok, None, 16, 1.0)[0]["iteration"][0] >= 0


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory for the rows and for the three results: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    rng = np.random.default_rng(10)
    pts, off = _sets(rng, [300, 0, 1030, 5], _two_view)
    models0, flags0, scores0 = ctx.ransac_fundamental(pts, off, 100, 1.0, 3, want_scores=True)
    _expect((models0, flags0, scores0), F.ransac(pts, off, 100, 1.0, 3))
    rows = pts.shape[0]
    # page-locked
    ppts = pinned_array(pts.shape, np.float32)
    ppts[...] = pts
    pm, pf, ps = pinned_array((4,), _lib.FUNDAMENTAL_DTYPE), pinned_array((rows,), np.uint8), pinned_array((4, 300), np.int32)
    ctx.ransac_fundamental(ppts, off, 100, 1.0, 3, models_out=pm, inlier_out=pf, scores_out=ps)
    assert F.same_bits(pm, models0) and F.same_bits(pf, flags0) and F.same_bits(ps, scores0)
    # device
    dpts = torch.from_numpy(pts).cuda()
    dm = torch.full((4, 12), 7, dtype=torch.int32, device="cuda")
    df = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
    ds = torch.full((4, 300), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ransac_fundamental(dpts, off, 100, 1.0, 3, models_out=dm, inlier_out=df, scores_out=ds)
    assert dm.cpu().numpy().tobytes() == models0.tobytes() and F.same_bits(df.cpu().numpy(), flags0)
    assert F.same_bits(ds.cpu().numpy(), scores0)
    # mixed: rows on the device, results to host memory, no scores asked
    models, flags = ctx.ransac_fundamental(dpts, off, 100, 1.0, 3)
    assert F.same_bits(models, models0) and F.same_bits(flags, flags0)


def _coords(kp, cnt, img, idx, scale):
    k = kp[(cnt[:img].sum() if img else 0) + idx]
    xy = np.stack([k["x"].astype(np.int64) << k["octave"], k["y"].astype(np.int64) << k["octave"]], axis=1).astype(np.float32)
    return xy * np.float32(scale)


def test_result_verify_fundamental_real_batch():
    """Two views of one frame 8 columns apart (the batch of test_result_verify_real_batch): sift_hip_result_verify_fundamental
    equals sift_hip_result_match plus the host loop on coordinates rebuilt in numpy, and the GPU call on them.  The pair is a
    pure shift, which does not determine F: only the identity of the results is asked, and that the winner explains more than
    the seven rows of its sample.  The default model still returns homographies."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    kp, _ = ctx.results()
    cnt = ctx.counts()
    pairs = [(0, 1), (1, 0)]
    for cross in (False, True):
        rec, counts, models, flags = ctx.verify_images(pairs, 0.8, cross, 512, 1.0, 19, model="fundamental")
        assert models.dtype == _lib.FUNDAMENTAL_DTYPE
        rec0, counts0 = ctx.match_images(pairs, 0.8, cross)
        assert F.same_bits(rec, rec0) and F.same_bits(counts, counts0) and flags.size == rec.size
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.zeros((rec.size, 4), np.float32)
        for p, (a, b) in enumerate(pairs):
            r = rec[off[p]:off[p + 1]]
            pts[off[p]:off[p + 1]] = np.concatenate([_coords(kp, cnt, a, r["query"], 1.0), _coords(kp, cnt, b, r["train"], 1.0)], axis=1)
        want = ctx.ransac_fundamental(pts, off, 512, 1.0, 19)
        assert F.same_bits(models, want[0]) and F.same_bits(flags, want[1])
        host = F.ransac(pts, off, 512, 1.0, 19)
        assert models.astype(F.MODEL_DTYPE).tobytes() == host[0].tobytes() and F.same_bits(flags, host[1])
        assert models["iteration"].min() >= 0 and models["inliers"][0] == flags[:counts[0]].sum() > 50
        print(f"cross {cross}: {counts.tolist()} matches, {models['inliers'].tolist()} inliers")
    with pytest.raises(ValueError):
        ctx.verify_images(pairs, refine=1, model="fundamental")
    with pytest.raises(ValueError):
        ctx.verify_images(pairs, model="affine")
    assert ctx.verify_images(pairs)[2].dtype == _lib.HOMOGRAPHY_DTYPE
    rec, counts, models, flags = ctx.verify_images([], model="fundamental")   # no pairs: nothing, and no error
    assert rec.size == 0 and models.size == 0
    ctx.close()


def test_sift_verify_wrapper():
    """Sift.verify(model="fundamental") = Sift.match + Context.ransac_fundamental on the points' image coordinates."""
    from sift_amd.sift import Sift
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    sift = Sift(3, 3)
    a = sift.calculate(np.ascontiguousarray(big[:, 0:256]))
    b = sift.calculate(np.ascontiguousarray(big[:, 8:264]))
    rec, model, flags = sift.verify(a, b, iterations=512, threshold=1.0, seed=19, model="fundamental")
    assert F.same_bits(rec, sift.match(a, b)) and flags.size == rec.size and model["inliers"] == flags.sum() > 50
    pts = np.array([[a[q].loc[0] << a[q].octave, a[q].loc[1] << a[q].octave, b[t].loc[0] << b[t].octave, b[t].loc[1] << b[t].octave]
                    for q, t in zip(rec["query"], rec["train"])], np.float32)
    want = F.ransac(pts, None, 512, 1.0, 19)
    assert np.asarray(model).reshape(1).astype(F.MODEL_DTYPE).tobytes() == want[0].tobytes() and F.same_bits(flags, want[1])
    with pytest.raises(ValueError):
        sift.verify(a, b, refine=1, model="fundamental")
    sift.ctx.close()


def test_cpp_example_and_cli_agree(tmp_path):
    """examples/sift_verify.cpp with model=fundamental (sift::Matcher::verify_fundamental) and `python -m sift_amd.cli --match ...
    --verify --model fundamental` write the same inliers.txt, byte for byte, and print the same F; --refine with it is an
    error."""
    import os
    import subprocess
    import sys
    from sift_amd import cli
    root = F.ROOT
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
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "2048", "3", "0", "0", "fundamental"], cwd=tmp_path / "cpp",
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "\nF " in out.stdout and "\nH " not in out.stdout, out.stdout + out.stderr
    cpp_f = [ln for ln in out.stdout.splitlines() if ln.startswith("F ")]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay", "--verify", "--model", "fundamental"]
    out = subprocess.run(base, cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "inliers" in out.stdout, out.stdout + out.stderr
    assert len(cpp_f) == 3 and [ln for ln in out.stdout.splitlines() if ln.startswith("F ")] == cpp_f
    got = open(tmp_path / "cpp" / "inliers.txt", "rb").read()
    assert got == open(tmp_path / "py" / "inliers.txt", "rb").read()
    matches = open(tmp_path / "cpp" / "matches.txt", "rb").read()
    assert matches == open(tmp_path / "py" / "matches.txt", "rb").read()
    lines, all_lines = got.decode().splitlines(), matches.decode().splitlines()
    assert 10 < len(lines) <= len(all_lines) and set(lines) <= set(all_lines)
    out = subprocess.run(base + ["--refine", "1"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--refine" in out.stderr
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "2048", "3", "0", "1", "fundamental"], cwd=tmp_path / "cpp",
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "refine" in out.stderr
