"""The GPU refinement of RANSAC homographies (ransac_refine_kernel behind sift_hip_ransac_homography's `refine`,
sift_hip_result_verify and sift_hip_refine_homography) against the host loop (tests/refine_ref.py: hostmath_refine_homography,
sift_amd/csrc/ransac_refine_math.h in plain loops, itself checked by tests/test_refine_host.py).  Every comparison is bitwise:
the model records with `refined`, and the flags."""
import numpy as np
import pytest

import ransac_ref as R
import refine_ref as F
from sift_amd import _lib

pytestmark = pytest.mark.gpu

# around the 256 partials of a fixed-order sum (one, exactly one and more than one row a lane) and the 1024-row scoring tile
SET_SIZES = [4, 5, 255, 256, 257, 1023, 1025, 2500]


def _noisy(rng, m):
    return R.projective_rows(rng, m, outliers=0.5 if m > 16 else 0.0, noise=0.5)[0]


def _sets(rng, sizes, gens):
    parts = [g(rng, m) for g, m in zip(gens, sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(parts).astype(np.float32).reshape(-1, 4), off


def _same(got, want, what=""):
    models, flags = got[0], got[1]
    assert np.asarray(models).tobytes() == want[0].tobytes(), (what, models, want[0])
    assert R.same_bits(np.asarray(flags), want[1]), what
    if len(got) > 2:
        assert R.same_bits(got[2], want[2]), what


@pytest.mark.parametrize("refine", [1, 3, 8])
def test_partial_edges(ctx, refine):
    """Every set size as the only set of a call and all of them as the sets of one call, 256 hypotheses, noisy rows."""
    rng = np.random.default_rng(40 + refine)
    pts, off = _sets(rng, SET_SIZES, [_noisy] * len(SET_SIZES))
    got = ctx.ransac_homography(pts, off, 256, 3.0, 5, want_scores=True, refine=refine)
    _same(got, F.ransac(pts, off, 256, 3.0, 5, refine=refine), "all")
    assert got[0]["refined"][2:].min() >= 1 and got[0]["refined"].max() <= refine
    for s, m in enumerate(SET_SIZES):
        rows = pts[off[s]:off[s + 1]]
        one = ctx.ransac_homography(rows, None, 256, 3.0, 5, want_scores=True, refine=refine)
        _same(one, F.ransac(rows, None, 256, 3.0, 5, refine=refine), m)


def _collinear(rng, m):
    """Forty rows on one horizontal line under a translation, the rest anywhere: whatever four-point model wins, its refit is
    the checker's, singular or not."""
    q = np.stack([np.floor(rng.random(40) * 1000), np.full(40, 300.0)], axis=1)
    return np.concatenate([np.concatenate([q, q + [5.0, 7.0]], axis=1), R.random_rows(rng, m - 40)]).astype(np.float32)


def test_nine_sets_one_call(ctx):
    rng = np.random.default_rng(50)
    sizes = [300, 0, 3, 700, 120, 90, 1025, 4, 64]
    gens = [_noisy, _noisy, _noisy, _noisy, R.random_rows, _collinear, _noisy, _noisy, _noisy]
    pts, off = _sets(rng, sizes, gens)
    for refine in (2, 8):
        got = ctx.ransac_homography(pts, off, 300, 3.0, 1, want_scores=True, refine=refine)
        _same(got, F.ransac(pts, off, 300, 3.0, 1, refine=refine), refine)
    models = got[0]
    assert (models["iteration"][[1, 2]] == -1).all() and (models["refined"][[1, 2]] == 0).all()
    assert models["refined"][[0, 3, 6]].min() >= 1
    base = ctx.ransac_homography(pts, off, 300, 3.0, 1)[0]
    assert (models["inliers"] >= base["inliers"]).all() and R.same_bits(models["iteration"], base["iteration"])


def _poor_model():
    t = R.apply_h(R.H_PROJ, F.CORNERS)
    t[2] += [2.5, -2.0]
    t[0] += [-1.5, 2.0]
    ok, h = R.homography4(np.concatenate([F.CORNERS, t], axis=1))
    assert ok
    return h


def test_refine_from_given_models(ctx):
    """sift_hip_refine_homography: a poor model that needs several rounds, a good one, one that is none, a collinear set with
    its translation (a singular solve), a set of three rows and an empty one."""
    rng = np.random.default_rng(60)
    sizes = [900, 400, 300, 100, 3, 0]
    pts, off = _sets(rng, sizes, [_noisy, _noisy, _noisy, _collinear, _noisy, _noisy])
    start = np.concatenate([F.model_of(_poor_model(), 11), F.model_of(R.H_PROJ, 0), F.model_of(R.H_PROJ, -1),
                            F.model_of([[1, 0, 5], [0, 1, 7], [0, 0, 1]], 2), F.model_of(R.H_PROJ, 4), F.model_of(R.H_PROJ, 9)])
    for rounds in (0, 1, 8):
        want = F.refine(pts, start, off, 3.0, rounds)
        got = ctx.refine_homography(pts, start.view(_lib.HOMOGRAPHY_DTYPE), off, 3.0, rounds)
        _same(got, want, rounds)
    models, flags = got
    assert models["refined"][0] >= 2                                      # the poor model gains inliers round after round
    assert models[2:3].tobytes() == start[2:3].tobytes() and not flags[off[2]:off[3]].any()
    assert models["refined"][3] == 0 and R.same_bits(models["h"][3], start["h"][3])
    assert R.same_bits(models["iteration"], start["iteration"])
    assert F.corner_error(models["h"][0]) < 1.0 < F.corner_error(start["h"][0])
    for bad in (dict(rounds=9), dict(rounds=-1), dict(threshold=0.0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            ctx.refine_homography(pts, start.view(_lib.HOMOGRAPHY_DTYPE), off, **bad)


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory for the rows, the models and the flags: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    rng = np.random.default_rng(70)
    pts, off = _sets(rng, [300, 0, 1030, 5], [_noisy] * 4)
    rows = pts.shape[0]
    want = F.ransac(pts, off, 300, 3.0, 3, refine=3)
    _same(ctx.ransac_homography(pts, off, 300, 3.0, 3, want_scores=True, refine=3), want)
    ppts = pinned_array(pts.shape, np.float32)
    ppts[...] = pts
    pm, pf = pinned_array((4,), _lib.HOMOGRAPHY_DTYPE), pinned_array((rows,), np.uint8)
    ctx.ransac_homography(ppts, off, 300, 3.0, 3, models_out=pm, inlier_out=pf, refine=3)
    _same((pm, pf), want)
    dpts = torch.from_numpy(pts).cuda()
    dm = torch.full((4, 12), 7, dtype=torch.int32, device="cuda")
    df = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.ransac_homography(dpts, off, 300, 3.0, 3, models_out=dm, inlier_out=df, refine=3)
    _same((dm.cpu().numpy(), df.cpu().numpy()), want)
    _same(ctx.ransac_homography(dpts, off, 300, 3.0, 3, refine=3), want)            # rows on the device, results to host memory
    # sift_hip_refine_homography: the models travel both ways
    start = F.ransac(pts, off, 300, 3.0, 3)[0]
    want = F.refine(pts, start, off, 3.0, 3)
    _same(ctx.refine_homography(pts, start.view(_lib.HOMOGRAPHY_DTYPE), off, 3.0, 3), want)
    pm[...] = start.view(_lib.HOMOGRAPHY_DTYPE)
    pf[...] = 9
    ctx.refine_homography(ppts, _lib_addr(pm), off, 3.0, 3, inlier_out=pf)
    _same((pm, pf), want)
    dm = torch.from_numpy(start.view(np.int32).reshape(4, 12).copy()).cuda()
    df = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.refine_homography(dpts, dm, off, 3.0, 3, inlier_out=df)
    _same((dm.cpu().numpy(), df.cpu().numpy()), want)
    host_models, host_flags = ctx.refine_homography(dpts, start.view(_lib.HOMOGRAPHY_DTYPE), off, 3.0, 3)
    _same((host_models, host_flags), want)


def _lib_addr(a):
    return int(a.ctypes.data)


def test_refine_range_and_zero(ctx):
    rng = np.random.default_rng(80)
    pts, off = _sets(rng, [500, 40], [_noisy, R.random_rows])
    with pytest.raises(ValueError):
        ctx.ransac_homography(pts, off, 64, 3.0, 0, refine=9)
    got = ctx.ransac_homography(pts, off, 64, 3.0, 0, want_scores=True, refine=0)
    want = R.ransac(pts, off, 64, 3.0, 0)
    assert got[0].astype(R.MODEL_DTYPE).tobytes() == want[0].tobytes() and R.same_bits(got[1], want[1]) and R.same_bits(got[2], want[2])
    assert (got[0]["refined"] == 0).all()
    _same(ctx.ransac_homography(pts, off, 64, 3.0, 0, want_scores=True, refine=8), F.ransac(pts, off, 64, 3.0, 0, refine=8))


def _coords(kp, cnt, img, idx, scale):
    k = kp[(cnt[:img].sum() if img else 0) + idx]
    xy = np.stack([k["x"].astype(np.int64) << k["octave"], k["y"].astype(np.int64) << k["octave"]], axis=1).astype(np.float32)
    return xy * np.float32(scale)


def test_result_verify_real_batch_refined():
    """The two images and parameters of test_result_verify_real_batch (two views of one frame 8 columns apart, seed 19, 2048
    hypotheses) with refine 2: sift_hip_result_verify equals sift_hip_result_match plus the checker on coordinates rebuilt in
    numpy.  `refined` >= 1 was confirmed on the CPU first for this seed (the oracle's descriptors, hostmath_match_knn2, the
    host loop): both pairs, without and with the cross-check, accept exactly one round at unchanged inlier counts (103, 97 and
    99, 94)."""
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
        rec, counts, models, flags = ctx.verify_images(pairs, 0.8, cross, 2048, 3.0, 19, refine=2)
        rec0, counts0 = ctx.match_images(pairs, 0.8, cross)
        assert R.same_bits(rec, rec0) and R.same_bits(counts, counts0) and flags.size == rec.size
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.zeros((rec.size, 4), np.float32)
        for p, (a, b) in enumerate(pairs):
            r = rec[off[p]:off[p + 1]]
            pts[off[p]:off[p + 1]] = np.concatenate([_coords(kp, cnt, a, r["query"], 1.0), _coords(kp, cnt, b, r["train"], 1.0)], axis=1)
        want = F.ransac(pts, off, 2048, 3.0, 19, refine=2)
        _same((models, flags), want, cross)
        _same(ctx.ransac_homography(pts, off, 2048, 3.0, 19, refine=2), want, cross)
        base = ctx.verify_images(pairs, 0.8, cross, 2048, 3.0, 19)[2]
        print(f"cross {cross}: {counts.tolist()} matches, inliers {base['inliers'].tolist()} -> {models['inliers'].tolist()}, "
              f"refined {models['refined'].tolist()}")
        assert (models["refined"] >= 1).all() and (models["inliers"] >= base["inliers"]).all()
        assert (base["refined"] == 0).all() and R.same_bits(models["iteration"], base["iteration"])
    with pytest.raises(ValueError):
        ctx.verify_images(pairs, refine=9)
    ctx.close()


def test_wrapper_cli_and_cpp_example_agree(tmp_path):
    """Sift.verify(refine=2), `python -m sift_amd.cli ... --verify --refine 2` and examples/sift_verify.cpp with its refine
    argument: the same model line for line, the same inliers.txt byte for byte, and the checker's model."""
    import os
    import subprocess
    import sys
    from sift_amd import cli
    from sift_amd.sift import Sift
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
    for d in ("cpp", "py"):
        (tmp_path / d).mkdir()
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "2048", "3", "0", "2"], cwd=tmp_path / "cpp", capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "\nH " in out.stdout and "\nrefined " in out.stdout, out.stdout + out.stderr
    cpp_lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("H ", "refined "))]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay"]
    out = subprocess.run(base + ["--verify", "--refine", "2"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    py_lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("H ", "refined "))]
    assert sorted(py_lines) == sorted(cpp_lines) and len(py_lines) == 4
    assert open(tmp_path / "cpp" / "inliers.txt", "rb").read() == open(tmp_path / "py" / "inliers.txt", "rb").read()
    out = subprocess.run(base + ["--refine", "2"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--refine needs --verify" in out.stderr
    # the wrapper, and the checker on its coordinates
    sift = Sift(3, 4)
    a = sift.calculate(img[:, :w - 8].astype(np.float32))
    b = sift.calculate(img[:, 8:].astype(np.float32))
    rec, model, flags = sift.verify(a, b, refine=2)
    pts = np.array([[a[q].loc[0] << a[q].octave, a[q].loc[1] << a[q].octave, b[t].loc[0] << b[t].octave, b[t].loc[1] << b[t].octave]
                    for q, t in zip(rec["query"], rec["train"])], np.float32)
    want = F.ransac(pts, None, 2048, 3.0, 0, refine=2)
    _same((np.asarray(model).reshape(1), flags), want)
    lines = ["H " + " ".join("%.9g" % float(v) for v in model["h"][3 * r:3 * r + 3]) for r in range(3)] + [f"refined {int(model['refined'])} rounds"]
    assert sorted(lines) == sorted(py_lines)
    base_rec, base_model, _ = sift.verify(a, b)
    assert R.same_bits(base_rec, rec) and base_model["refined"] == 0 and model["inliers"] >= base_model["inliers"]
    sift.ctx.close()
