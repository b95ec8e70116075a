"""GPU geometric verification (sift_hip_ransac_homography / sift_hip_result_verify) against the host loop
(tests/ransac_ref.py: hostmath_ransac_homography, sift_amd/csrc/ransac_math.h in plain loops, itself checked by
tests/test_ransac_host.py).  Every comparison is bitwise: the model records, the flags and the score of every hypothesis."""
import numpy as np
import pytest

import ransac_ref as R
from sift_amd import _lib

pytestmark = pytest.mark.gpu

# the issue's sizes plus the edges of the scoring kernel's tiles: 1024 rows of a set, 256 hypotheses
SET_SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 257, 1000, 1023, 1024, 1025, 2049]
ITERATIONS = [1, 63, 64, 65, 255, 256, 257, 513, 1000]


def _expect(got, want, what=""):
    models, flags, scores = got
    assert R.same_bits(scores, want[2]), (what, np.argwhere(scores != want[2])[:8].tolist())
    assert models.astype(R.MODEL_DTYPE).tobytes() == want[0].tobytes(), (what, models, want[0])
    assert R.same_bits(flags, want[1]), what


def _sets(rng, sizes, gen):
    parts = [gen(rng, m) for m in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(parts).astype(np.float32).reshape(-1, 4), off


def _projective(rng, m):
    return R.projective_rows(rng, m)[0]


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_tile_edges(ctx, iterations):
    """Every set size at every iteration count, the sizes as the sets of one call (a set's tiles are its own)."""
    rng = np.random.default_rng(100 + iterations)
    for gen in (_projective, R.random_rows):
        pts, off = _sets(rng, SET_SIZES, gen)
        got = ctx.ransac_homography(pts, off, iterations, 3.0, 5, want_scores=True)
        want = R.ransac(pts, off, iterations, 3.0, 5)
        _expect(got, want, gen.__name__)
        assert (got[0]["iteration"][:3] == -1).all() and (got[2][:3] == -1).all()
        if gen is _projective and iterations >= 255:
            assert (got[0]["inliers"][8:] >= 0.2 * np.array(SET_SIZES[8:])).all()   # the data's model is found: not a run of -1s


def test_many_sets_equal_each_alone(ctx):
    """A mix of sizes with empty sets in one call equals every set on its own - at the same set number, which enters the draw:
    a set alone is called with its number of empty sets in front of it."""
    rng = np.random.default_rng(7)
    sizes = [65, 0, 1000, 3, 0, 257, 1025, 4, 64]
    pts, off = _sets(rng, sizes, _projective)
    models, flags, scores = ctx.ransac_homography(pts, off, 300, 3.0, 1, want_scores=True)
    _expect((models, flags, scores), R.ransac(pts, off, 300, 3.0, 1))
    for s, m in enumerate(sizes):
        rows = pts[off[s]:off[s + 1]]
        one = ctx.ransac_homography(rows, [0] * (s + 1) + [m], 300, 3.0, 1, want_scores=True)
        assert R.same_bits(one[0][s:], models[s:s + 1]) and R.same_bits(one[1], flags[off[s]:off[s + 1]])
        assert R.same_bits(one[2][s], scores[s])
    # offsets that start above 0: the rows in front belong to no set
    got = ctx.ransac_homography(pts, off[2:], 300, 3.0, 1, want_scores=True)
    _expect(got, R.ransac(pts, off[2:], 300, 3.0, 1))
    assert not got[1][:off[2]].any()


def test_ties_go_to_the_lowest_iteration(ctx):
    """Two disjoint groups of 40 rows under two translations (exact in float): every sample from one group scores 40."""
    rng = np.random.default_rng(8)
    q = np.floor(rng.random((80, 2)) * 1000)
    t = q + np.where(np.arange(80)[:, None] < 40, [5.0, 7.0], [-30.0, 11.0])
    pts = np.concatenate([q, t], axis=1).astype(np.float32)[rng.permutation(80)]
    models, flags, scores = ctx.ransac_homography(pts, None, 512, 3.0, 0, want_scores=True)
    _expect((models, flags, scores), R.ransac(pts, None, 512, 3.0, 0))
    top = np.nonzero(scores[0] == scores[0].max())[0]
    assert scores[0].max() == 40 and top.size >= 8
    assert models[0]["iteration"] == top[0] and models[0]["inliers"] == 40 == flags.sum()
    # both groups are among the winners' equals: the tie is between different models
    shifts = {float(pts[R.draw(0, 0, int(i), 80)[0], 2] - pts[R.draw(0, 0, int(i), 80)[0], 0]) for i in top}
    assert shifts == {5.0, -30.0}


@pytest.mark.parametrize("m,iterations", [(40000, 3), (7, 65536)])
def test_split_independence(ctx, m, iterations):
    rng = np.random.default_rng(m)
    pts = _projective(rng, m)
    got = ctx.ransac_homography(pts, None, iterations, 3.0, 2, want_scores=True)
    _expect(got, R.ransac(pts, None, iterations, 3.0, 2))


def test_bad_values(ctx):
    rng = np.random.default_rng(9)
    pts = _projective(rng, 400)
    bad_rows = [3, 77, 130, 131, 399]
    pts[3, 0] = np.nan
    pts[77, 3] = np.inf
    pts[130, 1] = -np.inf
    pts[131] = np.nan
    pts[399, 2] = np.inf
    got = ctx.ransac_homography(pts, None, 256, 3.0, 4, want_scores=True)
    _expect(got, R.ransac(pts, None, 256, 3.0, 4))
    assert not got[1][bad_rows].any() and got[0]["inliers"][0] > 100
    ok = _projective(rng, 10)
    for kw in (dict(iterations=0), dict(iterations=65537), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")),
               dict(threshold=float("inf"))):
        with pytest.raises(ValueError):
            ctx.ransac_homography(ok, None, **kw)
    for off in ([0, 6, 5, 10], [-1, 10]):
        with pytest.raises(ValueError):
            ctx.ransac_homography(ok, off)
    assert ctx.ransac_homography(ok, None, 65536, 3.0)[0]["iteration"][0] >= 0


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory for the rows and for the three results: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    rng = np.random.default_rng(10)
    pts, off = _sets(rng, [300, 0, 1030, 5], _projective)
    models0, flags0, scores0 = ctx.ransac_homography(pts, off, 300, 3.0, 3, want_scores=True)
    _expect((models0, flags0, scores0), R.ransac(pts, off, 300, 3.0, 3))
    rows = pts.shape[0]
    # page-locked
    ppts = pinned_array(pts.shape, np.float32)
    ppts[...] = pts
    pm, pf, ps = pinned_array((4,), _lib.HOMOGRAPHY_DTYPE), pinned_array((rows,), np.uint8), pinned_array((4, 300), np.int32)
    ctx.ransac_homography(ppts, off, 300, 3.0, 3, models_out=pm, inlier_out=pf, scores_out=ps)
    assert R.same_bits(pm, models0) and R.same_bits(pf, flags0) and R.same_bits(ps, scores0)
    # device
    dpts = torch.from_numpy(pts).cuda()
    dm = torch.full((4, 12), 7, dtype=torch.int32, device="cuda")
    df = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
    ds = torch.full((4, 300), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ransac_homography(dpts, off, 300, 3.0, 3, models_out=dm, inlier_out=df, scores_out=ds)
    assert dm.cpu().numpy().tobytes() == models0.tobytes() and R.same_bits(df.cpu().numpy(), flags0)
    assert R.same_bits(ds.cpu().numpy(), scores0)
    # mixed: rows on the device, results to host memory, no scores asked
    models, flags = ctx.ransac_homography(dpts, off, 300, 3.0, 3)
    assert R.same_bits(models, models0) and R.same_bits(flags, flags0)


def _coords(kp, cnt, img, idx, scale):
    k = kp[(cnt[:img].sum() if img else 0) + idx]
    xy = np.stack([k["x"].astype(np.int64) << k["octave"], k["y"].astype(np.int64) << k["octave"]], axis=1).astype(np.float32)
    return xy * np.float32(scale)


def _verify_equals_match_plus_ransac(ctx, kp, cnt, pairs, ratio, cross, iterations, seed, scale):
    rec, counts, models, flags = ctx.verify_images(pairs, ratio, cross, iterations, 3.0, seed)
    rec0, counts0 = ctx.match_images(pairs, ratio, cross)
    assert R.same_bits(rec, rec0) and R.same_bits(counts, counts0) and flags.size == rec.size
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.zeros((rec.size, 4), np.float32)
    for p, (a, b) in enumerate(pairs):
        r = rec[off[p]:off[p + 1]]
        pts[off[p]:off[p + 1]] = np.concatenate([_coords(kp, cnt, a, r["query"], scale), _coords(kp, cnt, b, r["train"], scale)], axis=1)
    want = ctx.ransac_homography(pts, off, iterations, 3.0, seed)
    assert R.same_bits(models, want[0]) and R.same_bits(flags, want[1])
    host = R.ransac(pts, off, iterations, 3.0, seed)
    assert models.astype(R.MODEL_DTYPE).tobytes() == host[0].tobytes() and R.same_bits(flags, host[1])
    return rec, counts, models, flags


def test_result_verify_real_batch():
    """Two views of one frame 8 columns apart (the batch of test_real_descriptors_match_images): sift_hip_result_verify equals
    sift_hip_result_match plus sift_hip_ransac_homography on coordinates rebuilt in numpy, and the model of pair (0, 1) is the
    8-column shift.  That last condition was confirmed on the CPU first (the oracle's descriptors, hostmath_match_knn2, the
    host RANSAC loop): the list holds 126 matches (111 with the cross-check) of which 103 (99) lie within 3 px of the shift, but a
    slightly tilted model can collect one or two more, and does for most seeds at 2048 iterations; raising the iterations does
    not change that.  So the SEED was chosen: 19 is the first for which the host loop's winner is the exact shift both without
    and with the cross-check (corner deviation 0.0 px)."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    with pytest.raises(ValueError):
        ctx.verify_images([(0, 1)])                      # no results yet
    ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    kp, _ = ctx.results()
    cnt = ctx.counts()
    corners = np.array([[0, 0], [255, 0], [255, 191], [0, 191]], np.float64)
    for cross in (False, True):
        rec, counts, models, flags = _verify_equals_match_plus_ransac(ctx, kp, cnt, [(0, 1), (1, 0)], 0.8, cross, 2048, 19, 1.0)
        assert models["iteration"].min() >= 0 and models["inliers"][0] == flags[:counts[0]].sum() > 50
        dev = np.abs(R.apply_h(models[0]["h"], corners) - (corners + [-8, 0])).max()
        print(f"cross {cross}: {counts.tolist()} matches, {models['inliers'].tolist()} inliers, corner deviation {dev:.4f} px")
        assert dev <= 0.5
    with pytest.raises(ValueError):
        ctx.verify_images([(0, 2)])
    with pytest.raises(ValueError):
        ctx.verify_images([(0, 1)], iterations=0)
    rec, counts, models, flags = ctx.verify_images([])   # no pairs: nothing, and no error
    assert rec.size == 0 and models.size == 0
    # subpixel: the coordinates are those of the doubled image, halved
    ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 1))
    kp, _ = ctx.results()
    cnt = ctx.counts()
    rec, counts, models, flags = _verify_equals_match_plus_ransac(ctx, kp, cnt, [(0, 1)], 0.8, False, 512, 0, 0.5)
    assert models["iteration"][0] >= 0
    ctx.close()


def test_sift_verify_wrapper():
    """Sift.verify = Sift.match + Context.ransac_homography on the points' image coordinates."""
    from sift_amd.sift import Sift
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    sift = Sift(3, 3)
    a = sift.calculate(np.ascontiguousarray(big[:, 0:256]))
    b = sift.calculate(np.ascontiguousarray(big[:, 8:264]))
    rec, model, flags = sift.verify(a, b, seed=19)
    assert R.same_bits(rec, sift.match(a, b)) and flags.size == rec.size and model["inliers"] == flags.sum() > 50
    pts = np.array([[a[q].loc[0] << a[q].octave, a[q].loc[1] << a[q].octave, b[t].loc[0] << b[t].octave, b[t].loc[1] << b[t].octave]
                    for q, t in zip(rec["query"], rec["train"])], np.float32)
    want = R.ransac(pts, None, 2048, 3.0, 19)
    assert np.asarray(model).reshape(1).astype(R.MODEL_DTYPE).tobytes() == want[0].tobytes() and R.same_bits(flags, want[1])
    sift.ctx.close()


def test_cpp_example_and_cli_agree(tmp_path):
    """examples/sift_verify.cpp (sift::Matcher::verify) and `python -m sift_amd.cli --match ... --verify` write the same
    inliers.txt, byte for byte; without --verify the command writes the same matches.txt and no inliers.txt."""
    import os
    import subprocess
    import sys
    from sift_amd import cli
    root = R.ROOT
    exe = tmp_path / "sift_verify"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_verify.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    img = cli.read_image(os.path.join(root, "tests", "golden", "parrot_r.pgm")).astype(np.uint8)
    h, w = img.shape
    for name, part in (("a.pgm", img[:, :w - 8]), ("b.pgm", img[:, 8:])):
        with open(tmp_path / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w - 8, h) + np.ascontiguousarray(part).tobytes())
    for d in ("cpp", "py", "plain"):
        (tmp_path / d).mkdir()
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm"], cwd=tmp_path / "cpp", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "\nH " in out.stdout, out.stdout + out.stderr
    cpp_h = [ln for ln in out.stdout.splitlines() if ln.startswith("H ")]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay"]
    out = subprocess.run(base + ["--verify"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "inliers" in out.stdout, out.stdout + out.stderr
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("H ")] == cpp_h
    got = open(tmp_path / "cpp" / "inliers.txt", "rb").read()
    assert got == open(tmp_path / "py" / "inliers.txt", "rb").read()
    matches = open(tmp_path / "cpp" / "matches.txt", "rb").read()
    assert matches == open(tmp_path / "py" / "matches.txt", "rb").read()
    lines, all_lines = got.decode().splitlines(), matches.decode().splitlines()
    assert 10 < len(lines) <= len(all_lines) and set(lines) <= set(all_lines)
    out = subprocess.run(base, cwd=tmp_path / "plain", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "inliers" not in out.stdout, out.stdout + out.stderr
    assert matches == open(tmp_path / "plain" / "matches.txt", "rb").read()
    assert not os.path.exists(tmp_path / "plain" / "inliers.txt")
    out = subprocess.run([sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--verify"], cwd=tmp_path / "plain", capture_output=True,
                         text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--verify needs --match" in out.stderr
