"""GPU descriptor matching (sift_hip_knn2 / sift_hip_match / sift_hip_result_match) against the host checker
(tests/match_ref.py: hostmath_match_knn2, itself held to float64 by tests/test_match_host.py).  Every comparison is bitwise:
the indices and the bit patterns of the distances."""
import numpy as np
import pytest

import match_ref as M
from sift_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (2, 1), (1, 2), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127),
         (300, 2), (2, 300), (300, 300), (128, 33)]


def _expect(idx, dist, want):
    assert M.same_bits(idx, want[0]), np.nonzero((idx != want[0]).any(axis=1))[0][:8]
    assert M.same_bits(dist, want[1])


@pytest.mark.parametrize("gen", [M.desc_rows, M.uniform_rows], ids=["desc", "uniform"])
def test_tile_edges(ctx, gen):
    rng = np.random.default_rng(11)
    for nq, nt in SIZES:
        q, t = gen(rng, nq), gen(rng, nt)
        idx, dist = ctx.knn2(q, t)
        _expect(idx, dist, M.knn2(q, t))
        if nt == 1 and nq:
            assert (idx[:, 1] == -1).all() and np.isposinf(dist[:, 1]).all()


def test_mfma_layout():
    """Exact integer data whose distance matrix is asymmetric and different in every (i, j): one-hot query rows with their
    own scale against train rows that are permutations of 0 .. 127.  Every product and sum is exact in float32 in any order, so int64 numpy is a
    second, independent reference; a transposed or permuted tile, or a k-slice that was dropped, changes the nearest rows."""
    from sift_amd.sift import Context
    ctx = Context(0)
    rng = np.random.default_rng(3)
    nq, nt = 160, 100
    q = np.zeros((nq, 128), np.float32)
    q[np.arange(nq), (np.arange(nq) * 37) % 128] = np.arange(nq) % 23 + 1
    t = np.stack([rng.permutation(128) for _ in range(nt)]).astype(np.float32)   # equal norms: the products decide
    qi, ti = q.astype(np.int64), t.astype(np.int64)
    d = (qi * qi).sum(axis=1)[:, None] + (ti * ti).sum(axis=1)[None, :] - 2 * qi @ ti.T
    assert (d[:100, :100] != d[:100, :100].T).mean() > 0.9
    order = np.argsort(d, axis=1, kind="stable")
    idx, dist = ctx.knn2(q, t)
    assert (idx == order[:, :2]).all()
    assert (dist == np.take_along_axis(d, order[:, :2], axis=1).astype(np.float32)).all()
    assert np.unique(idx[:, 0]).size > 20
    _expect(idx, dist, M.knn2(q, t))
    idx, dist = ctx.knn2(t, q)
    order = np.argsort(d.T, axis=1, kind="stable")
    assert (idx == order[:, :2]).all()
    ctx.close()


def test_ties_and_duplicates(ctx):
    """Copies of a row on both sides of a stage edge (64 rows) and of a split edge (256 rows: with this few query rows the
    train set is cut at multiples of 256): the lower index is the best, the other copy the second, both at distance 0."""
    rng = np.random.default_rng(4)
    t = M.desc_rows(rng, 600)
    for a, b in ((63, 64), (255, 256), (10, 599), (511, 512)):
        t[b] = t[a]
    q = t[[63, 255, 10, 511, 7]]
    idx, dist = ctx.knn2(q, t)
    assert idx[:4].tolist() == [[63, 64], [255, 256], [10, 599], [511, 512]]
    assert (dist[:4] == 0).all() and idx[4, 0] == 7 and dist[4, 0] == 0
    _expect(idx, dist, M.knn2(q, t))
    # a set against itself: every row finds itself first, at exactly 0
    s = M.uniform_rows(rng, 333)
    idx, dist = ctx.knn2_sets(s, [0, 333], [(0, 0)])
    assert (idx[:, 0] == np.arange(333)).all() and (dist[:, 0] == 0).all()
    _expect(idx, dist, M.knn2(s, s))


def test_masks_nan_inf(ctx):
    rng = np.random.default_rng(6)
    q, t = M.desc_rows(rng, 140), M.desc_rows(rng, 150)
    qk, tk = np.zeros(140, _lib.KEYPOINT_DTYPE), np.zeros(150, _lib.KEYPOINT_DTYPE)
    qk["has_descriptor"] = rng.random(140) < 0.7
    tk["has_descriptor"] = rng.random(150) < 0.7
    t[5, 17] = np.nan
    t[9, 3] = np.inf
    q[11, 40] = np.nan
    tk["has_descriptor"][[5, 9]] = 1
    qk["has_descriptor"][11] = 1
    idx, dist = ctx.knn2(q, t, qk, tk)
    _expect(idx, dist, M.knn2(q, t, qk["has_descriptor"], tk["has_descriptor"]))
    bad = qk["has_descriptor"] == 0
    assert (idx[bad] == -1).all() and np.isposinf(dist[bad]).all()
    assert idx[11].tolist() == [-1, -1] and 5 not in idx.ravel().tolist()
    rec = ctx.match(q, t, 0.0, False, qk, tk)
    assert not np.isin(rec["query"], np.nonzero(bad)[0]).any() and 11 not in rec["query"].tolist()
    # only one side masked
    idx, dist = ctx.knn2(q, t, None, tk)
    _expect(idx, dist, M.knn2(q, t, None, tk["has_descriptor"]))


@pytest.mark.parametrize("nq,nt", [(3, 40000), (5000, 7)])
def test_split_independence(ctx, nq, nt):
    rng = np.random.default_rng(nq)
    q, t = M.uniform_rows(rng, nq), M.uniform_rows(rng, nt)
    idx, dist = ctx.knn2(q, t)
    _expect(idx, dist, M.knn2(q, t))


def _six_sets():
    rng = np.random.default_rng(8)
    sizes = [37, 130, 64, 0, 200, 5]
    sets = [M.desc_rows(rng, n) for n in sizes]
    sets[2][40] = sets[2][3]            # a duplicate inside the set that is matched against itself
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kp = np.zeros(off[-1], _lib.KEYPOINT_DTYPE)
    kp["has_descriptor"] = rng.random(off[-1]) < 0.9
    return sets, np.concatenate(sets), off, kp


PAIRS = [(0, 1), (1, 2), (2, 2), (5, 0), (3, 4)]


def test_many_pairs_one_call(ctx):
    sets, desc, off, kp = _six_sets()
    idx, dist = ctx.knn2_sets(desc, off, PAIRS, kp)
    r = 0
    for a, b in PAIRS:
        n = sets[a].shape[0]
        one = ctx.knn2_sets(desc, off, [(a, b)], kp)
        assert M.same_bits(idx[r:r + n], one[0]) and M.same_bits(dist[r:r + n], one[1])
        va, vb = kp["has_descriptor"][off[a]:off[a + 1]], kp["has_descriptor"][off[b]:off[b + 1]]
        _expect(one[0], one[1], M.knn2(sets[a], sets[b], va, vb))
        r += n
    assert r == idx.shape[0]


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 0.7, 0.8, 1.0])
def test_filtering(ctx, ratio, cross):
    sets, desc, off, kp = _six_sets()
    rec, counts = ctx.match_sets(desc, off, PAIRS, ratio, cross, kp)
    want = []
    for a, b in PAIRS:
        va, vb = kp["has_descriptor"][off[a]:off[a + 1]], kp["has_descriptor"][off[b]:off[b + 1]]
        fwd = M.knn2(sets[a], sets[b], va, vb)
        rev = M.knn2(sets[b], sets[a], vb, va)
        want.append(M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0]))
    assert counts.tolist() == [w.size for w in want]
    assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want))
    assert counts[4] == 0 and (ratio != 0.0 or cross or counts[0] == kp["has_descriptor"][off[0]:off[1]].sum())


def test_bad_ratio_is_einval(ctx):
    rng = np.random.default_rng(9)
    q = M.desc_rows(rng, 4)
    for ratio in (-1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.match(q, q, ratio)
    with pytest.raises(ValueError):
        ctx.knn2_sets(q, [0, 4], [(0, 1)])


def test_real_descriptors_match_images():
    """Two views of one frame 8 columns apart, as a batch of two: sift_hip_result_match on the device-resident results."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    with pytest.raises(ValueError):
        ctx.match_images([(0, 1)])                       # no results yet
    ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    kp, desc = ctx.results()
    cnt = ctx.counts()
    assert cnt.tolist() == [444, 441]
    sets = [desc[:cnt[0]], desc[cnt[0]:]]
    valid = [kp["has_descriptor"][:cnt[0]], kp["has_descriptor"][cnt[0]:]]
    for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
        rec, counts = ctx.match_images([(0, 1), (1, 0)], ratio, cross)
        want = []
        for a, b in ((0, 1), (1, 0)):
            fwd = M.knn2(sets[a], sets[b], valid[a], valid[b])
            rev = M.knn2(sets[b], sets[a], valid[b], valid[a])
            want.append(M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0]))
        assert counts.tolist() == [w.size for w in want]
        assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want))
        if ratio == 0.8 and not cross:   # a sanity line, not a threshold
            m = rec[:counts[0]]
            shifted = (np.abs(kp["x"][m["query"]].astype(int) * 2 ** kp["octave"][m["query"]].astype(int) - 8
                              - kp["x"][cnt[0] + m["train"]].astype(int) * 2 ** kp["octave"][cnt[0] + m["train"]].astype(int)) <= 2)
            print(f"ratio 0.8: {counts[0]} matches, {int(shifted.sum())} of them about 8 columns apart")
    with pytest.raises(ValueError):
        ctx.match_images([(0, 2)])
    ctx.close()


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory, for the inputs and for the results: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    sets, desc, off, kp = _six_sets()
    idx0, dist0 = ctx.knn2_sets(desc, off, PAIRS, kp)
    rec0, counts0 = ctx.match_sets(desc, off, PAIRS, 0.8, True, kp)
    rows = idx0.shape[0]
    # page-locked
    pdesc, pkp = pinned_array(desc.shape, np.float32), pinned_array(kp.shape, _lib.KEYPOINT_DTYPE)
    pdesc[...] = desc
    pkp[...] = kp
    pidx, pdist = pinned_array((rows, 2), np.int32), pinned_array((rows, 2), np.float32)
    ctx.knn2_sets(pdesc, off, PAIRS, pkp, pidx, pdist)
    assert M.same_bits(pidx, idx0) and M.same_bits(pdist, dist0)
    # device
    ddesc = torch.from_numpy(desc).cuda()
    dkp = torch.from_numpy(kp.view(np.uint8).reshape(-1, 20)).cuda()
    didx = torch.full((rows, 2), 7, dtype=torch.int32, device="cuda")
    ddist = torch.zeros((rows, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn2_sets(ddesc, off, PAIRS, dkp, didx, ddist)
    assert M.same_bits(didx.cpu().numpy(), idx0) and M.same_bits(ddist.cpu().numpy(), dist0)
    drec = torch.zeros((rows, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    total, counts = ctx.match_sets(ddesc, off, PAIRS, 0.8, True, dkp, recs_out=drec)
    assert total == rec0.size and counts.tolist() == counts0.tolist()
    assert drec.cpu().numpy()[:total].tobytes() == rec0.tobytes()
    # mixed: descriptors on the device, keypoints in host memory, results to host memory
    idx, dist = ctx.knn2_sets(ddesc, off, PAIRS, kp)
    assert M.same_bits(idx, idx0) and M.same_bits(dist, dist0)


def test_cpp_example_and_cli_agree(tmp_path):
    """examples/sift_match.cpp (sift::Matcher, include/sift/match.hpp) and `python -m sift_amd.cli --match` write the same
    matches.txt, byte for byte, for the parrot fixture against itself 8 columns on."""
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
    out = subprocess.run([str(exe), "../a.pgm", "../b.pgm"], cwd=tmp_path / "cpp", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "sift_amd.cli", "-i", "../a.pgm", "--match", "../b.pgm", "--no-overlay"], cwd=tmp_path / "py",
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "matches" in out.stdout, out.stdout + out.stderr
    got = open(tmp_path / "cpp" / "matches.txt", "rb").read()
    assert got == open(tmp_path / "py" / "matches.txt", "rb").read()
    lines = got.decode().splitlines()
    assert len(lines) > 10 and all(len(ln.split()) == 4 for ln in lines)
    assert [int(ln.split()[0]) for ln in lines] == sorted(int(ln.split()[0]) for ln in lines)
