"""GPU guided matching on 8-bit descriptors (sift_hip_knn2_guided_u8 / sift_hip_match_guided_u8 / sift_hip_result_match_guided_u8)
against numpy: match_u8_ref.dist_matrix (int64) as float32, guided_ref.admissible, guided_ref.top2, match_ref.filter_matches.
Every comparison is bitwise: the indices and the bit patterns of the distances."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guided_ref as G
import match_ref as M
import match_u8_ref as U
from sift_amd import _lib
from test_guided_gpu import NQ, NT, PAIRS, ZERO, _on_model, _six_sets
from test_guided_u8_host import knn2_u8_numpy as ref_knn2

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("kind", ["homography", "fundamental"])]


def _expect(got, want):
    assert G.same_bits(got[0], want[0]), np.nonzero((got[0] != want[0]).any(axis=1))[0][:8]
    assert G.same_bits(got[1], want[1])


def ref_matches(q, t, q_xy, t_xy, kind, model, thr, ratio, cross, q_valid=None, t_valid=None):
    fwd = ref_knn2(q, t, q_xy, t_xy, kind, model, thr, q_valid, t_valid)
    rev = ref_knn2(q, t, q_xy, t_xy, kind, model, thr, q_valid, t_valid, reverse=True)
    return M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0])


def test_tile_edges(ctx, kind):
    """The scenes of test_guided_gpu.py::test_tile_edges (same draws), at the scene's threshold and at a sixteenth of it, the
    narrow band in which whole wave-halves are skipped.  guided_ref.admissible on these draws: 2931 / 2916 of the 3367 query rows
    have an admissible row at the full threshold; 215 / 1840 at a sixteenth, with 413 / 104 of the 594 32 x 32 blocks empty."""
    rng = np.random.default_rng(31)
    found = [0, 0]
    for nq in NQ:
        for nt in NT:
            q, t = U.desc_rows_u8(rng, nq), U.desc_rows_u8(rng, nt)
            q_xy, t_xy, model, thr = G.banded_scene(rng, nq, nt, kind)
            for k, th in enumerate((thr, thr / 16)):
                got = ctx.knn2_guided_u8(q, t, q_xy, t_xy, model, kind, th)
                _expect(got, ref_knn2(q, t, q_xy, t_xy, kind, model, th))
                found[k] += int((got[0][:, 0] >= 0).sum())
    assert found[0] > 1000 and found[1] >= 100, found


@pytest.mark.parametrize("nq,nt", [(3, 40000), (5000, 7)])
def test_split_independence(ctx, kind, nq, nt):
    rng = np.random.default_rng(nq)
    q, t = U.uniform_rows_u8(rng, nq), U.uniform_rows_u8(rng, nt)
    q_xy, t_xy, model, thr = G.banded_scene(rng, nq, nt, kind)
    got = ctx.knn2_guided_u8(q, t, q_xy, t_xy, model, kind, thr)
    _expect(got, ref_knn2(q, t, q_xy, t_xy, kind, model, thr))
    assert (got[0][:, 0] >= 0).any()


def test_ties_and_extremes(ctx, kind):
    """Copies of a row on both sides of a stage edge (64) and of a split edge (256), both on the model: the lower index first,
    the other second, both at 0.  With one copy 150 px off only the copy in the band appears.  The extreme rows (0, 255, 127,
    128, alternating) among the train rows and as query rows: the sign flip and the range through the guided instantiation."""
    rng = np.random.default_rng(4)
    t = U.desc_rows_u8(rng, 600)
    q_xy, t_xy, model, _ = G.banded_scene(rng, 4, 600, kind)
    pairs = [(63, 64), (255, 256), (511, 512), (10, 599)]
    t[300:305] = U.EXTREMES
    for a, b in pairs:
        t[b] = t[a]
    q = t[[a for a, b in pairs]]
    spots = [_on_model(kind, model, q_xy[k]) for k in range(4)]
    for k, (a, b) in enumerate(pairs):
        t_xy[a] = t_xy[b] = spots[k]
    t_xy[300:305] = [spots[k % 4] for k in range(5)]     # the extremes compete
    idx, dist = ctx.knn2_guided_u8(q, t, q_xy, t_xy, model, kind, 3.0)
    assert idx.tolist() == [list(p) for p in pairs] and (dist == 0).all()
    _expect((idx, dist), ref_knn2(q, t, q_xy, t_xy, kind, model, 3.0))
    _expect(ctx.knn2_guided_u8(U.EXTREMES[:4], t, q_xy, t_xy, model, kind, 3.0), ref_knn2(U.EXTREMES[:4], t, q_xy, t_xy, kind, model, 3.0))
    for keep in (0, 1):
        xy = t_xy.copy()
        for k, p in enumerate(pairs):
            xy[p[1 - keep]] = spots[k] + [150.0, 170.0]
        idx, dist = ctx.knn2_guided_u8(q, t, q_xy, xy, model, kind, 3.0)
        assert idx[:, 0].tolist() == [p[keep] for p in pairs] and (dist[:, 0] == 0).all()
        assert all(idx[k, 1] != pairs[k][1 - keep] for k in range(4))
        _expect((idx, dist), ref_knn2(q, t, q_xy, xy, kind, model, 3.0))


def test_masks_bad_coordinates(ctx, kind):
    rng = np.random.default_rng(6)
    q, t = U.desc_rows_u8(rng, 140), U.desc_rows_u8(rng, 150)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 140, 150, kind)
    qk, tk = np.zeros(140, _lib.KEYPOINT_DTYPE), np.zeros(150, _lib.KEYPOINT_DTYPE)
    qk["has_descriptor"] = rng.random(140) < 0.7
    tk["has_descriptor"] = rng.random(150) < 0.7
    t_xy[20, 0], t_xy[21, 1], t_xy[22] = np.nan, np.inf, -np.inf
    q_xy[30, 1], q_xy[31, 0] = np.nan, np.inf
    tk["has_descriptor"][[20, 21, 22]] = 1
    qk["has_descriptor"][[30, 31]] = 1
    qv, tv = qk["has_descriptor"], tk["has_descriptor"]
    idx, dist = ctx.knn2_guided_u8(q, t, q_xy, t_xy, model, kind, thr, qk, tk)
    _expect((idx, dist), ref_knn2(q, t, q_xy, t_xy, kind, model, thr, qv, tv))
    assert (idx[qv == 0] == -1).all() and np.isposinf(dist[qv == 0]).all() and (idx[qv != 0, 0] >= 0).sum() > 20
    assert idx[30].tolist() == [-1, -1] and idx[31].tolist() == [-1, -1] and not np.isin(idx, [20, 21, 22]).any()
    rec = ctx.match_guided_u8(q, t, q_xy, t_xy, model, kind, thr, 0.0, True, qk, tk)      # the reverse best, bad rows on both sides
    want = ref_matches(q, t, q_xy, t_xy, kind, model, thr, 0.0, True, qv, tv)
    assert M.same_bits(rec.astype(want.dtype), want) and rec.size > 0


def test_zero_model_and_admit_all(ctx, kind):
    rng = np.random.default_rng(7)
    q, t = U.desc_rows_u8(rng, 140), U.desc_rows_u8(rng, 300)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 140, 300, kind)
    idx, dist = ctx.knn2_guided_u8(q, t, q_xy, t_xy, ZERO, kind, thr)
    assert (idx == -1).all() and np.isposinf(dist).all()
    assert ctx.match_guided_u8(q, t, q_xy, t_xy, ZERO, kind, 1e30, 0.0, False).size == 0
    every = G.IDENTITY if kind == "homography" else G.F_ADMIT_ALL
    _expect(ctx.knn2_guided_u8(q, t, q_xy, t_xy, every, kind, 1e30), ctx.knn2_u8(q, t))
    for ratio, cross in ((0.8, False), (0.9, True)):     # few records or none: random rows have no distinct nearest row
        assert ctx.match_guided_u8(q, t, q_xy, t_xy, every, kind, 1e30, ratio, cross).tobytes() == ctx.match_u8(q, t, ratio, cross).tobytes()


def test_many_pairs_one_call(ctx, kind):
    """The six sets of the float guided test (one empty, one matched against itself), as bytes; once more from device memory."""
    import torch
    fsets, _, xy, off, kp, models, thr = _six_sets(kind)
    sets = [U.quantize(s) for s in fsets]
    desc = np.concatenate(sets)
    part = lambda s: (sets[s], xy[off[s]:off[s + 1]], kp["has_descriptor"][off[s]:off[s + 1]])   # noqa: E731
    for ratio, cross in ((0.0, False), (0.0, True), (0.8, False), (0.8, True)):
        rec, counts = ctx.match_guided_sets_u8(desc, xy, off, PAIRS, models, kind, thr, ratio, cross, kp)
        want = []
        for p, (a, b) in enumerate(PAIRS):
            (qa, xa, va), (qb, xb, vb) = part(a), part(b)
            want.append(ref_matches(qa, qb, xa, xb, kind, models[p], thr, ratio, cross, va, vb))
        assert counts.tolist() == [w.size for w in want] and counts[4] == 0 and counts.sum() > 0
        assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want))
    ddesc, dxy, dmod = torch.from_numpy(desc).cuda(), torch.from_numpy(xy).cuda(), torch.from_numpy(models).cuda()
    dkp = torch.from_numpy(kp.view(np.uint8).reshape(-1, 20)).cuda()
    drec = torch.zeros((desc.shape[0], 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    total, counts = ctx.match_guided_sets_u8(ddesc, dxy, off, PAIRS, dmod, kind, thr, 0.8, True, dkp, recs_out=drec)
    assert total == rec.size and drec.cpu().numpy()[:total].tobytes() == rec.tobytes()
    with pytest.raises(ValueError, match="aligned"):
        ctx.knn2_guided_sets_u8(ddesc.data_ptr() + 8, dxy, off, PAIRS, dmod, kind, thr, dkp)


def test_real_batch(kind):
    """Two views of one frame 8 columns apart: sift_hip_result_match_guided_u8 under the models of verify_images equals
    match_guided_sets_u8 on results_u8() and the host-built coordinates, byte for byte - also with the localised coordinates."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    with pytest.raises(ValueError):
        ctx.match_images_guided_u8([(0, 1)], np.zeros((1, 9), np.float32))      # no results held
    pairs = [(0, 1), (1, 0)]
    thr = 3.0 if kind == "homography" else 1.0
    for subpixel in (0, 1):
        ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, subpixel))
        kp, d8 = ctx.results_u8()
        off = np.concatenate([[0], np.cumsum(ctx.counts())]).astype(np.int64)
        models = ctx.verify_images(pairs, 0.8, False, 512, thr, 19, model=kind)[2]
        assert (models["iteration"] >= 0).all()
        xy = np.stack([(kp["x"].astype(np.uint32) << kp["octave"]).astype(np.float32),
                       (kp["y"].astype(np.uint32) << kp["octave"]).astype(np.float32)], axis=1) * np.float32(0.5 if subpixel else 1.0)
        for localized in (False, True):
            if localized:
                loc = ctx.localize(use=True)
                xy = np.ascontiguousarray(np.stack([loc["x"], loc["y"]], axis=1), np.float32)
            for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
                rec, counts = ctx.match_images_guided_u8(pairs, models, kind, thr, ratio, cross, localized=localized)
                want, wcounts = ctx.match_guided_sets_u8(d8, xy, off, pairs, models, kind, thr, ratio, cross, kp)
                assert counts.tolist() == wcounts.tolist() and rec.tobytes() == want.tobytes() and counts.min() > 10
    for bad in (lambda: ctx.match_guided_sets_u8(d8, xy, off, pairs, models, kind, thr, quantized=2),
                lambda: ctx.match_guided_sets_u8(d8.astype(np.float32), xy, off, pairs, models, kind, thr),      # float rows
                lambda: ctx.knn2_guided_sets_u8(d8[:40], None, [0, 40], [(0, 0)], models[:1], kind, thr),        # NULL xy
                lambda: ctx.match_images_guided_u8(pairs, models[:1], kind, thr),                                # one model, two pairs
                lambda: ctx.match_images_guided(pairs, models, kind, thr, quantized=True)):                      # the float call
        with pytest.raises(ValueError):
            bad()
    assert ctx.match_guided_sets_u8(d8, xy, off, pairs, models, kind, thr, quantized=False)[0].size > 0
    ctx.close()


def test_cpp_example_and_cli_agree(tmp_path, kind):
    """examples/sift_guided.cpp with a trailing `u8` and `python -m sift_amd.cli --match ... --verify --guided-u8` write the same
    guided.txt, byte for byte; its distances are integers; --guided-u8 without --verify is an error."""
    from sift_amd import cli
    root = M.ROOT
    exe = tmp_path / "sift_guided"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_guided.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    img = cli.read_image(os.path.join(root, "tests", "golden", "parrot_r.pgm")).astype(np.uint8)
    h, w = img.shape
    for name, part in (("a.pgm", img[:, :w - 8]), ("b.pgm", img[:, 8:])):
        with open(tmp_path / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w - 8, h) + np.ascontiguousarray(part).tobytes())
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay"]
    run = lambda cmd, where: subprocess.run(cmd, cwd=tmp_path / where, capture_output=True, text=True, timeout=120, env=env)   # noqa: E731
    (tmp_path / "cpp").mkdir()
    (tmp_path / "py").mkdir()
    out = run([str(exe), "../a.pgm", "../b.pgm", kind, "u8"], "cpp")
    assert out.returncode == 0, out.stderr
    out = run(base + ["--verify", "--guided-u8", "--model", kind], "py")
    assert out.returncode == 0 and "guided" in out.stdout, out.stdout + out.stderr
    got = open(tmp_path / "cpp" / "guided.txt", "rb").read()
    assert got == open(tmp_path / "py" / "guided.txt", "rb").read()
    lines = got.decode().splitlines()
    assert len(lines) > 10 and all(ln.split()[2].isdigit() for ln in lines)
    out = run(base + ["--guided-u8"], "py")
    assert out.returncode != 0 and "--guided-u8 needs --verify" in out.stderr
