"""GPU guided matching (sift_hip_knn2_guided / sift_hip_match_guided / sift_hip_result_match_guided) against the host checker
(tests/guided_ref.py: hostmath_match_knn2_guided, itself held to a numpy restatement by tests/test_guided_host.py).  Every
comparison is bitwise: the indices and the bit patterns of the distances."""
import ctypes as C

import numpy as np
import pytest

import fund_ref as F
import guided_ref as G
import match_ref as M
import ransac_ref as R
from sift_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = ["homography", "fundamental"]
NQ = [1, 31, 32, 33, 127, 128, 129]
NT = [1, 63, 64, 65, 255, 256, 257]
ZERO = np.zeros(9, np.float32)


def _expect(got, want):
    assert G.same_bits(got[0], want[0]), np.nonzero((got[0] != want[0]).any(axis=1))[0][:8]
    assert G.same_bits(got[1], want[1])


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(ctx, kind):
    rng = np.random.default_rng(31)
    found = 0
    for nq in NQ:
        for nt in NT:
            q, t = M.desc_rows(rng, nq), M.desc_rows(rng, nt)
            q_xy, t_xy, model, thr = G.banded_scene(rng, nq, nt, kind)
            got = ctx.knn2_guided(q, t, q_xy, t_xy, model, kind, thr)
            _expect(got, G.knn2(q, t, q_xy, t_xy, kind, model, thr))
            found += int((got[0][:, 0] >= 0).sum())
    assert found > 1000     # the band is not empty


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq,nt", [(3, 40000), (5000, 7)])
def test_split_independence(ctx, kind, nq, nt):
    rng = np.random.default_rng(nq)
    q, t = M.uniform_rows(rng, nq), M.uniform_rows(rng, nt)
    q_xy, t_xy, model, thr = G.banded_scene(rng, nq, nt, kind)
    got = ctx.knn2_guided(q, t, q_xy, t_xy, model, kind, thr)
    _expect(got, G.knn2(q, t, q_xy, t_xy, kind, model, thr))
    assert (got[0][:, 0] >= 0).any()


def _on_model(kind, model, q_xy):
    """A train point that the query point admits: its transferred point / a point of its epipolar line."""
    line = np.asarray(model, np.float64).reshape(3, 3) @ [q_xy[0], q_xy[1], 1.0]
    return line[:2] / line[2] if kind == "homography" else np.array([900.0, -(line[0] * 900.0 + line[2]) / line[1]])


@pytest.mark.parametrize("kind", KINDS)
def test_ties_and_duplicates(ctx, kind):
    """Copies of a row on both sides of a stage edge (64 rows) and of a split edge (256 rows), the query row a third copy: with
    both copies at the admissible place the lower index is the best and the other the second, both at distance 0; with one of
    them elsewhere the one in the band is the best and the other copy appears nowhere."""
    rng = np.random.default_rng(4)
    t = M.desc_rows(rng, 600)
    q_xy, t_xy, model, _ = G.banded_scene(rng, 4, 600, kind)
    thr = 3.0
    pairs = [(63, 64), (255, 256), (10, 599), (511, 512)]
    for a, b in pairs:
        t[b] = t[a]
    q = t[[a for a, b in pairs]]
    for k, (a, b) in enumerate(pairs):
        t_xy[a] = t_xy[b] = _on_model(kind, model, q_xy[k])
    idx, dist = ctx.knn2_guided(q[:4], t, q_xy[:4], t_xy, model, kind, thr)
    assert idx.tolist() == [list(p) for p in pairs] and (dist == 0).all()
    _expect((idx, dist), G.knn2(q[:4], t, q_xy[:4], t_xy, kind, model, thr))
    for first in (True, False):
        xy = t_xy.copy()
        for k in range(4):
            a, b = pairs[k]
            spot = _on_model(kind, model, q_xy[k])
            xy[a], xy[b] = (spot, spot + [150.0, 170.0]) if first else (spot + [150.0, 170.0], spot)
        idx, dist = ctx.knn2_guided(q[:4], t, q_xy[:4], xy, model, kind, thr)
        assert idx[:, 0].tolist() == [p[0 if first else 1] for p in pairs] and (dist[:, 0] == 0).all()
        for k in range(4):
            assert idx[k, 1] != pairs[k][1 if first else 0]
        _expect((idx, dist), G.knn2(q[:4], t, q_xy[:4], xy, kind, model, thr))


@pytest.mark.parametrize("kind", KINDS)
def test_masks_nan_inf(ctx, kind):
    rng = np.random.default_rng(6)
    q, t = M.desc_rows(rng, 140), M.desc_rows(rng, 150)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 140, 150, kind)
    qk, tk = np.zeros(140, _lib.KEYPOINT_DTYPE), np.zeros(150, _lib.KEYPOINT_DTYPE)
    qk["has_descriptor"] = rng.random(140) < 0.7
    tk["has_descriptor"] = rng.random(150) < 0.7
    t[5, 17] = np.nan
    t[9, 3] = np.inf
    q[11, 40] = np.nan
    t_xy[20, 0] = np.nan
    t_xy[21, 1] = np.inf
    t_xy[22] = -np.inf
    q_xy[30, 1] = np.nan
    q_xy[31, 0] = np.inf
    tk["has_descriptor"][[5, 9, 20, 21, 22]] = 1
    qk["has_descriptor"][[11, 30, 31]] = 1
    got = ctx.knn2_guided(q, t, q_xy, t_xy, model, kind, thr, qk, tk)
    _expect(got, G.knn2(q, t, q_xy, t_xy, kind, model, thr, qk["has_descriptor"], tk["has_descriptor"]))
    idx, dist = got
    bad = qk["has_descriptor"] == 0
    assert (idx[bad] == -1).all() and np.isposinf(dist[bad]).all()
    assert idx[11].tolist() == [-1, -1] and idx[30].tolist() == [-1, -1] and idx[31].tolist() == [-1, -1]
    assert not np.isin(idx, [5, 20, 21, 22]).any()
    # no masks, and one side only
    _expect(ctx.knn2_guided(q, t, q_xy, t_xy, model, kind, thr), G.knn2(q, t, q_xy, t_xy, kind, model, thr))
    _expect(ctx.knn2_guided(q, t, q_xy, t_xy, model, kind, thr, None, tk), G.knn2(q, t, q_xy, t_xy, kind, model, thr, None, tk["has_descriptor"]))
    # the reverse best with bad coordinates on both sides: through the cross-check
    rec = ctx.match_guided(q, t, q_xy, t_xy, model, kind, thr, 0.0, True, qk, tk)
    want = G.matches(q, t, q_xy, t_xy, kind, model, thr, 0.0, True, qk["has_descriptor"], tk["has_descriptor"])
    assert M.same_bits(rec.astype(want.dtype), want) and rec.size > 0


@pytest.mark.parametrize("kind", KINDS)
def test_zero_model_and_admit_all(ctx, kind):
    rng = np.random.default_rng(7)
    q, t = M.desc_rows(rng, 140), M.desc_rows(rng, 300)
    q_xy, t_xy, model, thr = G.banded_scene(rng, 140, 300, kind)
    idx, dist = ctx.knn2_guided(q, t, q_xy, t_xy, ZERO, kind, thr)
    assert (idx == -1).all() and np.isposinf(dist).all()
    assert ctx.match_guided(q, t, q_xy, t_xy, ZERO, kind, 1e30, 0.0, False).size == 0
    every = G.IDENTITY if kind == "homography" else G.F_ADMIT_ALL
    got = ctx.knn2_guided(q, t, q_xy, t_xy, every, kind, 1e30)
    _expect(got, ctx.knn2(q, t))
    _expect(got, M.knn2(q, t))
    for ratio, cross in ((0.8, False), (0.9, True)):
        assert ctx.match_guided(q, t, q_xy, t_xy, every, kind, 1e30, ratio, cross).tobytes() == ctx.match(q, t, ratio, cross).tobytes()


PAIRS = [(0, 1), (1, 2), (2, 2), (5, 0), (3, 4), (1, 0)]


def _six_sets(kind):
    rng = np.random.default_rng(8)
    sizes = [37, 130, 64, 0, 200, 5]
    sets = [M.desc_rows(rng, n) for n in sizes]
    sets[2][40] = sets[2][3]            # a duplicate inside the set that is matched against itself
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kp = np.zeros(off[-1], _lib.KEYPOINT_DTYPE)
    kp["has_descriptor"] = rng.random(off[-1]) < 0.9
    if kind == "homography":            # every pair its own shift of a 60 px square; 12 px admit about a tenth
        xy = (400.0 + rng.random((off[-1], 2)) * 60.0).astype(np.float32)
        models = np.tile(G.IDENTITY, (len(PAIRS), 1))
        models[:, 2] = rng.uniform(-10, 10, len(PAIRS))
        models[:, 5] = rng.uniform(-10, 10, len(PAIRS))
        thr = 12.0
    else:                               # every pair its own two-view scene
        xy = (rng.random((off[-1], 2)) * F.SIZE).astype(np.float32)
        models = np.stack([F.two_view_scene(rng)[2].ravel() for _ in PAIRS]).astype(np.float32)
        thr = 100.0
    return sets, np.concatenate(sets), np.ascontiguousarray(xy), off, kp, np.ascontiguousarray(models, np.float32), thr


def _set(s, sets, xy, off, kp):
    return sets[s], xy[off[s]:off[s + 1]], kp["has_descriptor"][off[s]:off[s + 1]]


@pytest.mark.parametrize("kind", KINDS)
def test_many_pairs_one_call(ctx, kind):
    sets, desc, xy, off, kp, models, thr = _six_sets(kind)
    idx, dist = ctx.knn2_guided_sets(desc, xy, off, PAIRS, models, kind, thr, kp)
    r = 0
    for p, (a, b) in enumerate(PAIRS):
        (qa, xa, va), (qb, xb, vb) = _set(a, sets, xy, off, kp), _set(b, sets, xy, off, kp)
        n = qa.shape[0]
        _expect((idx[r:r + n], dist[r:r + n]), G.knn2(qa, qb, xa, xb, kind, models[p], thr, va, vb))
        r += n
    assert r == idx.shape[0] and (idx[:, 0] >= 0).sum() > 100
    # the same pair under two models in one call: the models are the pairs', not the sets'
    two = np.stack([models[0], models[5]])
    idx2, dist2 = ctx.knn2_guided_sets(desc, xy, off, [(0, 1), (0, 1)], two, kind, thr, kp)
    assert G.same_bits(idx2[:37], idx[:37]) and not G.same_bits(idx2[37:], idx[:37])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 0.8, 1.0])
def test_filtering(ctx, kind, ratio, cross):
    sets, desc, xy, off, kp, models, thr = _six_sets(kind)
    rec, counts = ctx.match_guided_sets(desc, xy, off, PAIRS, models, kind, thr, ratio, cross, kp)
    want = []
    for p, (a, b) in enumerate(PAIRS):
        (qa, xa, va), (qb, xb, vb) = _set(a, sets, xy, off, kp), _set(b, sets, xy, off, kp)
        want.append(G.matches(qa, qb, xa, xb, kind, models[p], thr, ratio, cross, va, vb))
    assert counts.tolist() == [w.size for w in want]
    assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want))
    assert counts[4] == 0 and counts.sum() > 0     # the comparison above is not one of empty lists


def test_pointer_kinds(ctx):
    """Pageable, page-locked and device memory for desc, xy, models and the results: identical bytes."""
    import torch
    from sift_amd.sift import pinned_array
    kind = "homography"
    sets, desc, xy, off, kp, models, thr = _six_sets(kind)
    idx0, dist0 = ctx.knn2_guided_sets(desc, xy, off, PAIRS, models, kind, thr, kp)
    rec0, counts0 = ctx.match_guided_sets(desc, xy, off, PAIRS, models, kind, thr, 0.8, True, kp)
    rows = idx0.shape[0]
    assert rec0.size > 0
    # page-locked
    pdesc, pxy, pmod = pinned_array(desc.shape, np.float32), pinned_array(xy.shape, np.float32), pinned_array(models.shape, np.float32)
    pdesc[...], pxy[...], pmod[...] = desc, xy, models
    pidx, pdist = pinned_array((rows, 2), np.int32), pinned_array((rows, 2), np.float32)
    ctx.knn2_guided_sets(pdesc, pxy, off, PAIRS, pmod, kind, thr, kp, pidx, pdist)
    assert M.same_bits(pidx, idx0) and M.same_bits(pdist, dist0)
    # device
    ddesc, dxy, dmod = torch.from_numpy(desc).cuda(), torch.from_numpy(xy).cuda(), torch.from_numpy(models).cuda()
    dkp = torch.from_numpy(kp.view(np.uint8).reshape(-1, 20)).cuda()
    didx = torch.full((rows, 2), 7, dtype=torch.int32, device="cuda")
    ddist = torch.zeros((rows, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn2_guided_sets(ddesc, dxy, off, PAIRS, dmod, kind, thr, dkp, didx, ddist)
    assert M.same_bits(didx.cpu().numpy(), idx0) and M.same_bits(ddist.cpu().numpy(), dist0)
    drec = torch.zeros((rows, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    total, counts = ctx.match_guided_sets(ddesc, dxy, off, PAIRS, dmod, kind, thr, 0.8, True, dkp, recs_out=drec)
    assert total == rec0.size and counts.tolist() == counts0.tolist()
    assert drec.cpu().numpy()[:total].tobytes() == rec0.tobytes()
    # mixed: each of xy / models alone on the device, the rest and the results in host memory
    for use_xy, use_mod in ((dxy, models), (xy, dmod), (dxy, pmod)):
        idx, dist = ctx.knn2_guided_sets(desc, use_xy, off, PAIRS, use_mod, kind, thr, kp)
        assert M.same_bits(idx, idx0) and M.same_bits(dist, dist0)


def test_parameter_rejections(ctx):
    """Each is SIFT_HIP_EINVAL with a message, and nothing is written."""
    rng = np.random.default_rng(9)
    q = M.desc_rows(rng, 4)
    xy = np.ascontiguousarray(rng.random((4, 2)), np.float32)
    off = np.array([0, 4], np.int64)
    p0 = np.zeros(1, np.int32)
    L, h = ctx._L, ctx._h
    idx, dist = np.full((4, 2), 9, np.int32), np.zeros((4, 2), np.float32)
    rec = np.zeros(4, _lib.MATCH_DTYPE)
    mod = np.ascontiguousarray(G.IDENTITY)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731

    def knn(guide, xy_=xy, mod_=mod):
        err = C.create_string_buffer(256)
        rc = L.sift_hip_knn2_guided(h, vp(q), None, vp(xy_), 1, off, 1, p0, p0, None if guide is None else C.byref(guide), vp(mod_), vp(idx),
                                    vp(dist), err, 256)
        return rc, err.value

    def match(guide, ratio=0.8, xy_=xy, mod_=mod):
        err = C.create_string_buffer(256)
        prm = _lib.MatchParams(ratio, 0)
        rc = L.sift_hip_match_guided(h, vp(q), None, vp(xy_), 1, off, 1, p0, p0, C.byref(prm), None if guide is None else C.byref(guide),
                                     vp(mod_), vp(rec), p0.copy(), None, err, 256)
        return rc, err.value
    good = _lib.GuideParams(0, 3.0)
    assert knn(good)[0] == _lib.OK and match(good)[0] == _lib.OK
    idx[...] = 9
    bad = [_lib.GuideParams(2, 3.0), _lib.GuideParams(0xffffffff, 3.0)]
    bad += [_lib.GuideParams(1, v) for v in (0.0, -1.0, float("nan"), float("inf"), float("-inf"))]
    for call in (knn, match):
        for g in bad + [None]:
            rc, msg = call(g)
            assert rc == _lib.EINVAL and msg, (g and (g.model, g.threshold))
        for kw in ({"xy_": None}, {"mod_": None}):
            rc, msg = call(good, **kw)
            assert rc == _lib.EINVAL and msg, kw
    for ratio in (-1.0, 1.5, float("nan")):
        rc, msg = match(good, ratio)
        assert rc == _lib.EINVAL and msg
    assert (idx == 9).all()
    # the wrappers: a ValueError
    with pytest.raises(ValueError):
        ctx.knn2_guided(q, q, xy, xy, mod, "affine", 3.0)
    with pytest.raises(ValueError):
        ctx.knn2_guided(q, q, xy, xy, mod, "homography", 0.0)
    with pytest.raises(ValueError):
        ctx.knn2_guided_sets(q, xy, off, [(0, 1)], mod.reshape(1, 9), "homography", 3.0)       # a set that does not exist
    with pytest.raises(ValueError):
        ctx.knn2_guided_sets(q, xy, off, [(0, 0)], np.zeros((2, 9), np.float32), "homography", 3.0)   # two models, one pair


@pytest.mark.parametrize("kind", KINDS)
def test_real_batch(kind):
    """Two views of one frame 8 columns apart, as a batch of two: sift_hip_result_match_guided under the models of
    verify_images equals match_guided_sets on the downloaded descriptors and coordinates, and every record satisfies the host
    predicate."""
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx = Context(0)
    with pytest.raises(ValueError):
        ctx.match_images_guided([(0, 1)], np.zeros((1, 9), np.float32))      # no results yet
    pairs = [(0, 1), (1, 0)]
    inlier_fn = R.inlier if kind == "homography" else F.inlier
    for subpixel in (0, 1):
        ctx.calculate_batch(imgs, _lib.Params(3, 3, 1.6, K_SQRT2, subpixel))
        kp, desc = ctx.results()
        cnt = ctx.counts()
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        thr = 3.0 if kind == "homography" else 1.0
        _, _, models, _ = ctx.verify_images(pairs, 0.8, False, 512, thr, 19, model=kind)
        assert (models["iteration"] >= 0).all()
        xy = np.stack([(kp["x"].astype(np.uint32) << kp["octave"]).astype(np.float32),
                       (kp["y"].astype(np.uint32) << kp["octave"]).astype(np.float32)], axis=1) * np.float32(0.5 if subpixel else 1.0)
        for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
            rec, counts = ctx.match_images_guided(pairs, models, kind, thr, ratio, cross)
            want, wcounts = ctx.match_guided_sets(desc, xy, off, pairs, models, kind, thr, ratio, cross, kp)
            assert counts.tolist() == wcounts.tolist() and rec.tobytes() == want.tobytes()
            assert counts.min() > 10
            r = 0
            for p, (a, b) in enumerate(pairs):
                m9 = models[p]["h" if kind == "homography" else "f"]
                for one in rec[r:r + counts[p]]:
                    row = np.concatenate([xy[off[a] + one["query"]], xy[off[b] + one["train"]]])
                    assert inlier_fn(m9, row, thr)
                r += counts[p]
        # against the host checker, one pair
        a, b = pairs[0]
        want = G.matches(desc[off[a]:off[a + 1]], desc[off[b]:off[b + 1]], xy[off[a]:off[a + 1]], xy[off[b]:off[b + 1]], kind,
                         models[0]["h" if kind == "homography" else "f"], thr, 0.8, True,
                         kp["has_descriptor"][off[a]:off[a + 1]], kp["has_descriptor"][off[b]:off[b + 1]])
        rec, counts = ctx.match_images_guided([pairs[0]], models[:1], kind, thr, 0.8, True)
        assert M.same_bits(rec.astype(want.dtype), want)
    # a pair without a winner: all zeros, no records
    none = models.copy()
    none["h" if kind == "homography" else "f"][1] = 0
    rec, counts = ctx.match_images_guided(pairs, none, kind, thr, 0.0, False)
    assert counts[1] == 0 and counts[0] > 0
    with pytest.raises(ValueError):
        ctx.match_images_guided([(0, 2)], models[:1], kind, thr)
    ctx.close()


def test_sift_match_guided_wrapper():
    from sift_amd.sift import Sift
    from sift_amd.synthetic import synth_frame
    big = synth_frame(272, 192, 1)
    s = Sift(3, 3)
    a = s.calculate(np.ascontiguousarray(big[:, 0:256]))
    b = s.calculate(np.ascontiguousarray(big[:, 8:264]))
    for kind, thr in (("homography", 3.0), ("fundamental", 1.0)):
        recs, model, inlier = s.verify(a, b, threshold=thr, model=kind)
        assert model["iteration"] >= 0
        guided = s.match_guided(a, b, model, thr, 0.8, False)
        # every verified inlier is still there: its partner was the nearest of all rows and is admissible, and the second best
        # among fewer rows is no nearer than it was
        keep = recs[inlier != 0]
        assert keep.size > 10 and guided.size >= keep.size
        at = np.searchsorted(guided["query"], keep["query"])
        assert (guided["query"][at] == keep["query"]).all() and (guided["train"][at] == keep["train"]).all()
        assert s.match_guided(a, b, model, thr, 0.8, True).size <= guided.size
    with pytest.raises(ValueError):
        s.match_guided(a, b, np.zeros(9, np.float32))
    s.ctx.close()


def test_cpp_example_and_cli_agree(tmp_path):
    """examples/sift_guided.cpp (sift::Matcher::match_guided) and `python -m sift_amd.cli --match ... --verify --guided` write
    the same guided.txt, byte for byte, for both models; --guided without --verify is an error."""
    import os
    import subprocess
    import sys
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
    for kind in KINDS:
        cpp, py = tmp_path / ("cpp_" + kind), tmp_path / ("py_" + kind)
        cpp.mkdir()
        py.mkdir()
        out = subprocess.run([str(exe), "../a.pgm", "../b.pgm", kind], cwd=cpp, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        out = subprocess.run(base + ["--verify", "--guided", "--model", kind], cwd=py, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0 and "guided" in out.stdout, out.stdout + out.stderr
        got = open(cpp / "guided.txt", "rb").read()
        assert got == open(py / "guided.txt", "rb").read()
        assert open(cpp / "matches.txt", "rb").read() == open(py / "matches.txt", "rb").read()
        lines = got.decode().splitlines()
        assert len(lines) > 10 and all(len(ln.split()) == 4 for ln in lines)
        assert len(lines) >= len(open(py / "inliers.txt").read().splitlines()) // 2
    (tmp_path / "plain").mkdir()
    out = subprocess.run(base + ["--guided"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--guided needs --verify" in out.stderr
