"""8-bit descriptors and integer matching on the GPU (sift_hip_quantize, sift_hip_result_copy_u8, sift_hip_knn2_u8,
sift_hip_match_u8 and sift_hip_match_params.quantized) against the host checker (tests/match_u8_ref.py, itself held to int64
numpy by tests/test_match_u8_host.py).  Every comparison is bitwise: the indices and the bit patterns of the distances."""
import numpy as np
import pytest

import match_ref as M
import match_u8_ref as U
from sift_amd import _lib
from test_match_gpu import PAIRS, SIZES

pytestmark = pytest.mark.gpu


def _expect(got, want):
    assert M.same_bits(got[0], want[0]), np.nonzero((got[0] != want[0]).any(axis=1))[0][:8]
    assert M.same_bits(got[1], want[1])


@pytest.fixture(scope="module")
def two_crops():
    """Two views of one frame 8 columns apart, as a batch of two (the batch of test_match_gpu.py), in a context of its own:
    (context, keypoints, float descriptors, counts)."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    c = Context(0)
    c.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    kp, desc = c.results()
    yield c, kp, desc, c.counts()
    c.close()


def test_quantize_parity(ctx):
    import torch
    from sift_amd.sift import pinned_array
    rng = np.random.default_rng(1)
    kat = np.zeros(128, np.float32)
    kat[:U.KAT_IN.size] = U.KAT_IN
    for rows in (0, 1, 63, 64, 65, 4097):
        d = (rng.random((rows, 128)) * 1.2 - 0.1).astype(np.float32)
        if rows:
            d[rows // 2] = kat
        want = U.quantize(d)
        got = ctx.quantize(d)
        assert got.dtype == np.uint8 and M.same_bits(got, want), rows
        if rows == 0:
            continue
        dd = torch.from_numpy(d).cuda()
        out = torch.full((rows, 128), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.quantize(dd, out)
        assert M.same_bits(out.cpu().numpy(), want), rows
        pd, pout = pinned_array(d.shape, np.float32), pinned_array(d.shape, np.uint8)
        pd[...] = d
        ctx.quantize(pd, pout)
        assert M.same_bits(pout, want), rows
        assert M.same_bits(ctx.quantize(dd), want)                       # device in, host out
    assert (ctx.quantize(kat)[0, :U.KAT_IN.size] == U.KAT_OUT).all()


@pytest.mark.parametrize("gen", [U.desc_rows_u8, U.uniform_rows_u8], ids=["desc", "uniform"])
def test_tile_edges(ctx, gen):
    rng = np.random.default_rng(11)
    for nq, nt in SIZES + [(65, 63), (63, 65), (64, 64)]:
        q, t = gen(rng, nq), gen(rng, nt)
        idx, dist = ctx.knn2_u8(q, t)
        _expect((idx, dist), U.knn2(q, t))
        if nt == 1 and nq:
            assert (idx[:, 1] == -1).all() and np.isposinf(dist[:, 1]).all()


def test_mfma_layout(ctx):
    """Exact asymmetric data: one-hot query rows with their own scale against train rows that are permutations of 0 .. 127, both
    ways round, against int64 numpy.  A transposed tile, a dropped k-slice or A and B operands that disagree on which k a lane's
    bytes are change the nearest rows.  This is what establishes the C/D map of the i8 instruction, not the guide."""
    rng = np.random.default_rng(3)
    nq, nt = 160, 100
    q = np.zeros((nq, 128), np.uint8)
    q[np.arange(nq), (np.arange(nq) * 37) % 128] = np.arange(nq) % 23 + 1
    t = np.stack([rng.permutation(128) for _ in range(nt)]).astype(np.uint8)   # equal norms: the products decide
    d = U.dist_matrix(q, t)
    assert (d[:100, :100] != d[:100, :100].T).mean() > 0.9
    for a, b, dm in ((q, t, d), (t, q, d.T)):
        order = np.argsort(dm, axis=1, kind="stable")
        idx, dist = ctx.knn2_u8(a, b)
        assert (idx == order[:, :2]).all()
        assert (dist == np.take_along_axis(dm, order[:, :2], axis=1).astype(np.float32)).all()
        _expect((idx, dist), U.knn2(a, b))
    assert np.unique(ctx.knn2_u8(q, t)[0][:, 0]).size > 20


def test_extremes_and_ties(ctx):
    e = U.EXTREMES
    idx, dist = ctx.knn2_u8(e, e)
    _expect((idx, dist), U.knn2(e, e))
    assert (idx[:, 0] == np.arange(5)).all() and (dist[:, 0] == 0).all()
    idx, dist = ctx.knn2_u8(e[:1], e[1:2])
    assert idx.tolist() == [[0, -1]] and dist[0, 0] == 8323200 and np.isposinf(dist[0, 1])
    # each extreme row alone against the other four, embedded in a stage's worth of them
    big = np.concatenate([e[(np.arange(70) + 1) % 5], e])
    _expect(ctx.knn2_u8(e, big), U.knn2(e, big))
    # copies on both sides of a stage edge (64) and of a split edge (256): the lower index first, the copy second, both at 0
    rng = np.random.default_rng(4)
    t = U.desc_rows_u8(rng, 600)
    for a, b in ((63, 64), (255, 256), (10, 599), (511, 512)):
        t[b] = t[a]
    q = t[[63, 255, 10, 511, 7]]
    idx, dist = ctx.knn2_u8(q, t)
    assert idx[:4].tolist() == [[63, 64], [255, 256], [10, 599], [511, 512]]
    assert (dist[:4] == 0).all() and idx[4, 0] == 7 and dist[4, 0] == 0
    _expect((idx, dist), U.knn2(q, t))
    # 300 identical train rows: every candidate ties, the order of the indices decides
    same = np.repeat(t[:1], 300, axis=0)
    idx, dist = ctx.knn2_u8(t[:40], same)
    assert (idx == [0, 1]).all() and (dist[:, 0] == dist[:, 1]).all()
    _expect((idx, dist), U.knn2(t[:40], same))


@pytest.mark.parametrize("nq,nt", [(3, 40000), (5000, 7)])
def test_split_independence(ctx, nq, nt):
    rng = np.random.default_rng(nq)
    q, t = U.uniform_rows_u8(rng, nq), U.uniform_rows_u8(rng, nt)
    _expect(ctx.knn2_u8(q, t), U.knn2(q, t))


def _six_sets(lead=0):
    """Six sets (one empty, one matched against itself with a duplicate inside), some rows without a descriptor; `lead` rows in
    front that belong to no set (offsets that start above 0)."""
    rng = np.random.default_rng(8)
    sizes = [37, 130, 64, 0, 200, 5]
    sets = [U.desc_rows_u8(rng, n) for n in sizes]
    sets[2][40] = sets[2][3]
    off = (np.concatenate([[0], np.cumsum(sizes)]) + lead).astype(np.int64)
    desc = np.concatenate([U.uniform_rows_u8(rng, lead)] + sets)
    kp = np.zeros(off[-1], _lib.KEYPOINT_DTYPE)
    kp["has_descriptor"] = rng.random(off[-1]) < 0.9
    return sets, desc, off, kp


@pytest.mark.parametrize("lead", [0, 19])
def test_many_pairs_masks_offsets(ctx, lead):
    sets, desc, off, kp = _six_sets(lead)
    idx, dist = ctx.knn2_sets_u8(desc, off, PAIRS, kp)
    r = 0
    for a, b in PAIRS:
        n = sets[a].shape[0]
        one = ctx.knn2_sets_u8(desc, off, [(a, b)], kp)
        assert M.same_bits(idx[r:r + n], one[0]) and M.same_bits(dist[r:r + n], one[1])
        va, vb = kp["has_descriptor"][off[a]:off[a + 1]], kp["has_descriptor"][off[b]:off[b + 1]]
        _expect(one, U.knn2(sets[a], sets[b], va, vb))
        assert (one[0][va == 0] == -1).all()
        r += n
    assert r == idx.shape[0]


def _want_records(sets, off, kp, ratio, cross):
    want = []
    for a, b in PAIRS:
        va, vb = kp["has_descriptor"][off[a]:off[a + 1]], kp["has_descriptor"][off[b]:off[b + 1]]
        fwd = U.knn2(sets[a], sets[b], va, vb)
        rev = U.knn2(sets[b], sets[a], vb, va)
        want.append(M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0]))
    return want


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 0.7, 0.8, 1.0])
def test_filtering(ctx, ratio, cross):
    sets, desc, off, kp = _six_sets()
    rec, counts = ctx.match_sets_u8(desc, off, PAIRS, ratio, cross, kp)
    want = _want_records(sets, off, kp, ratio, cross)
    assert counts.tolist() == [w.size for w in want]
    assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want))
    assert counts[4] == 0 and (ratio != 0.0 or cross or counts[0] == kp["has_descriptor"][off[0]:off[1]].sum())


def _image_sets(kp, rows, cnt):
    return [rows[:cnt[0]], rows[cnt[0]:]], [kp["has_descriptor"][:cnt[0]], kp["has_descriptor"][cnt[0]:]]


def test_flag_equals_quantize_then_match(ctx, two_crops):
    # float rows with the flag = the bytes of quantize() through the byte call
    rng = np.random.default_rng(8)
    sizes = [37, 130, 64, 0, 200, 5]
    fdesc = M.desc_rows(rng, sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kp = np.zeros(off[-1], _lib.KEYPOINT_DTYPE)
    kp["has_descriptor"] = rng.random(off[-1]) < 0.9
    q8 = ctx.quantize(fdesc)
    assert M.same_bits(q8, U.quantize(fdesc))
    for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
        a = ctx.match_sets(fdesc, off, PAIRS, ratio, cross, kp, quantized=True)
        b = ctx.match_sets_u8(q8, off, PAIRS, ratio, cross, kp)
        assert M.same_bits(a[0], b[0]) and a[1].tolist() == b[1].tolist() and a[0].size > 0
        want = _want_records([q8[off[i]:off[i + 1]] for i in range(6)], off, kp, ratio, cross)
        assert M.same_bits(a[0].astype(want[0].dtype), np.concatenate(want))
    assert M.same_bits(ctx.match(fdesc[:37], fdesc[37:167], 0.8, True, quantized=True), ctx.match_u8(q8[:37], q8[37:167], 0.8, True))

    # the device-resident results of a real batch
    c, kp, desc, cnt = two_crops
    kp8, d8 = c.results_u8()
    assert M.same_bits(kp8, kp) and d8.shape == (kp.size, 128) and M.same_bits(d8, U.quantize(desc))
    off = np.array([0, cnt[0], cnt[0] + cnt[1]], np.int64)
    pairs = [(0, 1), (1, 0)]
    for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
        rec, counts = c.match_images(pairs, ratio, cross, quantized=True)
        rec2, counts2 = c.match_sets_u8(d8, off, pairs, ratio, cross, kp)
        assert M.same_bits(rec, rec2) and counts.tolist() == counts2.tolist() and rec.size > 0

    # verification over the 8-bit matches: the match above plus the RANSAC call on the rebuilt coordinates
    for model in ("homography", "fundamental"):
        rec, counts, models, inlier = c.verify_images(pairs, 0.8, True, 256, 3.0, 5, model=model, quantized=True)
        rec2, counts2 = c.match_sets_u8(d8, off, pairs, 0.8, True, kp)
        assert M.same_bits(rec, rec2) and counts.tolist() == counts2.tolist()
        pts, r = [], 0
        for p, (a, b) in enumerate(pairs):
            m = rec[r:r + counts[p]]
            ka, kb = kp[off[a] + m["query"]], kp[off[b] + m["train"]]
            pts.append(np.stack([(ka["x"].astype(np.uint32) << ka["octave"]).astype(np.float32),
                                 (ka["y"].astype(np.uint32) << ka["octave"]).astype(np.float32),
                                 (kb["x"].astype(np.uint32) << kb["octave"]).astype(np.float32),
                                 (kb["y"].astype(np.uint32) << kb["octave"]).astype(np.float32)], axis=1))
            r += counts[p]
        run = c.ransac_fundamental if model == "fundamental" else c.ransac_homography
        models2, inlier2 = run(np.concatenate(pts), np.concatenate([[0], np.cumsum(counts)]), 256, 3.0, 5)
        assert M.same_bits(models, models2) and M.same_bits(inlier, inlier2)
        assert models["inliers"].min() > 20


def test_agrees_with_float_matching(two_crops):
    """Ratio 0.8, no cross-check, first image against the second.  The CPU comparison of the float64 distances with the integer
    ones on this batch: 126 float records, 125 8-bit records, all 125 with the float record's train row.  The bounds (95 % of the
    float records reappear with the same train row; at most 5 % more records) leave room for the f32 chain's distances to move a
    handful of borderline ratio tests relative to float64."""
    c, kp, desc, cnt = two_crops
    f32, _ = c.match_images([(0, 1)], 0.8, False)
    u8, _ = c.match_images([(0, 1)], 0.8, False, quantized=True)
    train8 = dict(zip(u8["query"].tolist(), u8["train"].tolist()))
    again = sum(1 for q, t in zip(f32["query"].tolist(), f32["train"].tolist()) if train8.get(q) == t)
    print(f"ratio 0.8: {f32.size} float records, {u8.size} 8-bit records, {again} float records reappear with the same train row")
    assert f32.size > 50
    assert again >= 0.95 * f32.size
    assert u8.size <= 1.05 * f32.size


def test_errors(ctx, two_crops):
    rng = np.random.default_rng(9)
    q = M.desc_rows(rng, 40)
    q8 = U.quantize(q)
    with pytest.raises(ValueError):
        ctx.match(q, q, 0.8, quantized=2)
    xy = (rng.random((80, 2)) * 100).astype(np.float32)
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    with pytest.raises(ValueError, match="guided"):
        ctx.match_guided_sets(np.concatenate([q, q]), xy, [0, 40, 80], [(0, 1)], eye, quantized=True)
    assert ctx.match_guided_sets(np.concatenate([q, q]), xy, [0, 40, 80], [(0, 1)], eye, threshold=1e6)[0].size > 0
    c = two_crops[0]
    with pytest.raises(ValueError, match="guided"):
        c.match_images_guided([(0, 1)], eye, quantized=True)
    with pytest.raises(ValueError):
        c.match_images([(0, 1)], quantized=3)
    for ratio in (-1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.match_u8(q8, q8, ratio)
        with pytest.raises(ValueError):
            ctx.match(q, q, ratio, quantized=True)
    with pytest.raises(ValueError):
        ctx.knn2_sets_u8(q8, [0, 4], [(0, 1)])
    with pytest.raises(ValueError):
        ctx.knn2_u8(q, q)                                # float rows are not converted silently
    # the f32 default still is the float definition
    _expect(ctx.knn2(q, q[:30]), M.knn2(q, q[:30]))
    assert M.same_bits(ctx.match(q, q[:30], 0.8), ctx.match(q, q[:30], 0.8, quantized=False))


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory, for the rows and for the results: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    sets, desc, off, kp = _six_sets()
    idx0, dist0 = ctx.knn2_sets_u8(desc, off, PAIRS, kp)
    rec0, counts0 = ctx.match_sets_u8(desc, off, PAIRS, 0.8, True, kp)
    rows = idx0.shape[0]
    pdesc, pkp = pinned_array(desc.shape, np.uint8), pinned_array(kp.shape, _lib.KEYPOINT_DTYPE)
    pdesc[...] = desc
    pkp[...] = kp
    pidx, pdist = pinned_array((rows, 2), np.int32), pinned_array((rows, 2), np.float32)
    ctx.knn2_sets_u8(pdesc, off, PAIRS, pkp, pidx, pdist)
    assert M.same_bits(pidx, idx0) and M.same_bits(pdist, dist0)
    ddesc = torch.from_numpy(desc).cuda()
    dkp = torch.from_numpy(kp.view(np.uint8).reshape(-1, 20)).cuda()
    didx = torch.full((rows, 2), 7, dtype=torch.int32, device="cuda")
    ddist = torch.zeros((rows, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn2_sets_u8(ddesc, off, PAIRS, dkp, didx, ddist)
    assert M.same_bits(didx.cpu().numpy(), idx0) and M.same_bits(ddist.cpu().numpy(), dist0)
    drec = torch.zeros((rows, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    total, counts = ctx.match_sets_u8(ddesc, off, PAIRS, 0.8, True, dkp, recs_out=drec)
    assert total == rec0.size and counts.tolist() == counts0.tolist()
    assert drec.cpu().numpy()[:total].tobytes() == rec0.tobytes()
    idx, dist = ctx.knn2_sets_u8(ddesc, off, PAIRS, kp)
    assert M.same_bits(idx, idx0) and M.same_bits(dist, dist0)
    # float rows on the device with the flag
    fdesc = M.desc_rows(np.random.default_rng(5), int(off[-1]))
    want = ctx.match_sets_u8(ctx.quantize(fdesc), off, PAIRS, 0.8, True, kp)
    got = ctx.match_sets(torch.from_numpy(fdesc).cuda(), off, PAIRS, 0.8, True, dkp, quantized=True)
    assert M.same_bits(got[0], want[0]) and got[1].tolist() == want[1].tolist()
    # a device address that is not aligned to 16 bytes is refused, not read
    with pytest.raises(ValueError, match="aligned"):
        ctx.knn2_sets_u8(ddesc.data_ptr() + 8, off, PAIRS, kp)


def test_cpp_example_and_cli_agree(tmp_path):
    """examples/sift_match.cpp with quantized = 1 and `python -m sift_amd.cli --match --u8` write the same matches.txt, byte for
    byte; the distances print as the integers they are.  --u8 with --guided is refused by name."""
    import os
    import subprocess
    import sys
    from sift_amd import cli
    root = M.ROOT
    exe = tmp_path / "sift_match"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_match.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    img = cli.read_image(os.path.join(root, "tests", "golden", "parrot_r.pgm")).astype(np.uint8)
    h, w = img.shape
    for name, part in (("a.pgm", img[:, :w - 8]), ("b.pgm", img[:, 8:])):
        with open(tmp_path / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w - 8, h) + np.ascontiguousarray(part).tobytes())
    (tmp_path / "cpp").mkdir()
    (tmp_path / "py").mkdir()
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", "4", "3", "0.8", "0", "1"], cwd=tmp_path / "cpp", capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--u8", "--no-overlay"],
                         cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "matches" in out.stdout, out.stdout + out.stderr
    got = open(tmp_path / "cpp" / "matches.txt", "rb").read()
    assert got == open(tmp_path / "py" / "matches.txt", "rb").read()
    lines = got.decode().splitlines()
    assert len(lines) > 10 and all(len(ln.split()) == 4 for ln in lines)
    assert all(ln.split()[2].isdigit() and (ln.split()[3].isdigit() or ln.split()[3] == "inf") for ln in lines)
    out = subprocess.run([sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--u8", "--verify", "--guided",
                          "--no-overlay"], cwd=tmp_path / "py", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--u8" in out.stderr
